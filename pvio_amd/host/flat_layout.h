// flat_layout.h -- the ONE copy of how a Frame's members cross into the flat arrays of the C ABI and of PnpProblem, and back.
// The layouts are those of include/pvio_hip.h (pvio_ba_problem / pvio_ba_state; pnp_problem.h uses the same ones); every matrix crosses
// element by element (the ABI is row-major, Eigen column-major).  Written against host_seam.h: the reference's own types inside the PVIO
// tree, the look-alikes of the standalone tests otherwise.  tests/host/roundtrip.cpp keeps inverse helpers of its own on purpose: it is
// the independent side of the flatten -> Map -> flatten round trip.
#pragma once
#include "host_seam.h"

namespace pvio {
namespace flat {

inline void put_q(double *dst, const quaternion &q) { // x y z w
    for (int k = 0; k < 4; ++k) dst[k] = q.coeffs()[k];
}
inline void put_m3(double *dst, const matrix<3> &m) { // -> row-major
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) dst[3 * r + c] = m(r, c);
}

// state [16] (pvio_ba_state::frame_state, pvio_ba_problem::prior_lin_state): q(xyzw) p v bg ba
inline void put_state(double *s, const PoseState &pose, const MotionState &motion) {
    put_q(s, pose.q);
    for (int k = 0; k < 3; ++k) s[4 + k] = pose.p[k], s[7 + k] = motion.v[k], s[10 + k] = motion.bg[k], s[13 + k] = motion.ba[k];
}
inline void put_state(double *s, const Frame *f) { put_state(s, f->pose, f->motion); }
// ... and back, in place: the pose always, the motion only where the solve had motion blocks
inline void write_back_state(const double *s, Frame *f, bool with_motion) {
    for (int k = 0; k < 4; ++k) f->pose.q.coeffs()[k] = s[k];
    for (int k = 0; k < 3; ++k) f->pose.p[k] = s[4 + k];
    if (with_motion)
        for (int k = 0; k < 3; ++k) f->motion.v[k] = s[7 + k], f->motion.bg[k] = s[10 + k], f->motion.ba[k] = s[13 + k];
}

// extrinsic [7] (cam_extrinsic, imu_extrinsic): q_cs(xyzw) p_cs
inline void put_extrinsic(double *e, const ExtrinsicParams &x) {
    put_q(e, x.q_cs);
    for (int k = 0; k < 3; ++k) e[4 + k] = x.p_cs[k];
}
// sqrt_inv_cov [4]: frame->sqrt_inv_cov, 2x2 row-major
inline void put_sqrt_inv_cov(double *c, const matrix<2> &m) { c[0] = m(0, 0), c[1] = m(0, 1), c[2] = m(1, 0), c[3] = m(1, 1); }
// intrinsics [4]: fx fy cx cy of frame->K
inline void put_intrinsics(double *i, const matrix<3> &K) { i[0] = K(0, 0), i[1] = K(1, 1), i[2] = K(0, 2), i[3] = K(1, 2); }

// pre-integration (preint_delta [11]: dt dq(xyzw) dp dv; preint_sqrt_inv_cov [225]: 15x15 row-major; preint_jacobian [45]: dq_dbg dp_dbg
// dp_dba dv_dbg dv_dba, 3x3 row-major each)
inline void put_preintegration(double *delta, double *U, double *jac, const PreIntegrator &pre) {
    const PreIntegrator::Delta &d = pre.delta;
    delta[0] = d.t;
    put_q(delta + 1, d.q);
    for (int k = 0; k < 3; ++k) delta[5 + k] = d.p[k], delta[8 + k] = d.v[k];
    for (int r = 0; r < 15; ++r)
        for (int c = 0; c < 15; ++c) U[15 * r + c] = d.sqrt_inv_cov(r, c);
    const PreIntegrator::Jacobian &j = pre.jacobian;
    put_m3(jac, j.dq_dbg), put_m3(jac + 9, j.dp_dbg), put_m3(jac + 18, j.dp_dba), put_m3(jac + 27, j.dv_dbg), put_m3(jac + 36, j.dv_dba);
}

} // namespace flat
} // namespace pvio
