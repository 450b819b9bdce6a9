// hip_buffer.h -- the owner of one grow-only scratch allocation (host code only), in device memory (hipMalloc / hipFree) or in pinned host memory
// (hipHostMalloc / hipHostFree).  No names, no pool: DevicePool (ba_solver.h, keyed by name) and Klt::slab_pool_ (reuse by exact size) do other jobs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace pvhip {

template <bool kPinned>
class ScratchBuffer {
  public:
    ScratchBuffer() = default;
    ScratchBuffer(const ScratchBuffer &) = delete;
    ScratchBuffer &operator=(const ScratchBuffer &) = delete;
    ~ScratchBuffer() { release(); }
    // The buffer, once it holds `need` (> 0) bytes.  One that is large enough is kept as it is; otherwise it is freed FIRST (the peak is one
    // buffer, not two; the contents are scratch) and `grow_to` >= need bytes are allocated: the headroom is the caller's policy.
    // nullptr: the allocation failed, the owner is empty (capacity 0) and a later call tries again.
    void *reserve(size_t need, size_t grow_to) {
        if (need <= cap_) return ptr_;
        release();
        if (grow_to < need) grow_to = need;
        if ((kPinned ? hipHostMalloc(&ptr_, grow_to) : hipMalloc(&ptr_, grow_to)) != hipSuccess) return ptr_ = nullptr;
        cap_ = grow_to;
        return ptr_;
    }
    void *data() const { return ptr_; }
    template <class T>
    T *as() const { return static_cast<T *>(ptr_); }
    size_t capacity() const { return cap_; } // bytes

  private:
    void release() {
        if (ptr_) (void)(kPinned ? hipHostFree(ptr_) : hipFree(ptr_));
        ptr_ = nullptr, cap_ = 0;
    }
    void *ptr_ = nullptr;
    size_t cap_ = 0;
};
using DeviceBuffer = ScratchBuffer<false>;
using PinnedBuffer = ScratchBuffer<true>;

} // namespace pvhip
