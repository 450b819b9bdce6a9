"""Independent numpy restatement of pvio_hip_plane_ransac (include/pvio_hip.h; pvio_amd/csrc/pv_plane.h, ba_plane.hip) and the helpers of
tests/test_plane_ransac.py.

reference(points, ...) is the sequential algorithm of Ransac<3, PlaneState, PlaneSolver, PlaneEvaluator> (utility/ransac.h,
core/plane_extractor.h:47-65) followed by the refit of plane_extractor.cpp:59-77:
  sampler      minstd_rand0 (x <- 16807 x mod (2^31 - 1), seed 0 -> 1) under libstdc++'s uniform_int_distribution (range 2^31 - 3, buckets of
               range // m, redraw past m buckets) under a LotBox whose permutation persists over iterations; plain Python integers
  model/error  numpy float64 scalars and element-wise array operations, one IEEE operation each (numpy does not contract), in the order
               (x0 y0 + x1 y1) + x2 y2: the same bits as pv_plane.h
  bookkeeping  strictly more inliers replace the best; N = K / log(1 - ratio^5) shrinks iter_max (math.log / pow)
  refit        cog and scatter with numpy sums, the eigenvector with numpy.linalg.eigh (LAPACK, not Jacobi), the sign rule of the header

margin(points, ...) is the smallest | error - threshold | over every hypothesis the sequential loop looks at and every point: a case is STRICT
only if the restatement alone gives margin >= STRICT_MARGIN = 1e-9 -- errors are sums of three products of numbers of a few metres, so two
correct implementations differ by a few 1e-16 and cannot flip a decision.

Refit tolerances, computed from the restatement alone (count = number of inliers, eps = 2^-52):
  cog            4 count eps max|p|                       (a sum of `count` terms in any order: count eps max|p|, divided by count exactly once)
  refit_normal   4 count eps trace(cov) / (l1 - l0) + 16 eps   (|d cov| <= count eps trace-sized terms against the eigenvalue gap -- Davis-Kahan --;
                                                                16 eps for the Jacobi rotations and the normalization)
  refit_distance |cog| tol_normal + tol_cog + 4 eps |cog|       (normal . cog)
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

EPS = 2.0 ** -52
STRICT_MARGIN = 1e-9
M31 = 2147483647


class Sampler:
    def __init__(self, n, seed):
        self.lots = list(range(n))
        self.x = seed % M31 or 1

    def _next(self):
        self.x = self.x * 16807 % M31
        return self.x

    def _uniform(self, a, b):
        m = b - a + 1
        scaling = 2147483645 // m
        past = m * scaling
        while True:
            r = self._next() - 1
            if r < past:
                return a + r // scaling

    def sample(self):
        lots, n, out = self.lots, len(self.lots), []
        for cap in range(3):
            if n - cap > 1:
                j = self._uniform(cap, n - 1)
                lots[cap], lots[j] = lots[j], lots[cap]
                out.append(lots[cap])
            else:
                out.append(lots[-1])
        return out


def dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def model(p0, p1, p2):
    """(normal [3], distance) of plane_extractor.h:47-55 with Eigen's stableNormalize"""
    with np.errstate(all="ignore"):
        a, b = p2 - p0, p1 - p0
        c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        w = abs(c[0])
        for k in (1, 2):
            if abs(c[k]) > w:
                w = abs(c[k])
        s = c / w
        z = dot(s, s)
        if z > 0:
            c = c / (np.sqrt(z) * w)
        return c, dot(p0, c)


def errors(points, normal, distance):
    with np.errstate(all="ignore"):
        return np.abs(((points[:, 0] * normal[0] + points[:, 1] * normal[1]) + points[:, 2] * normal[2]) - distance)


def orient(v, toward):
    d = dot(v, toward)
    if d < 0 or (d == 0 and tuple(v[v != 0][:1] < 0) == (True,)):
        return -v
    return v


def reference(points, threshold=0.03, confidence=0.999, max_iterations=1000, seed=0, want_margin=False):
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = len(points)
    res = dict(n_inliers=0, iterations=0, best_iteration=-1, refit_valid=0, inlier_mask=np.zeros(n, np.uint8), normal=np.zeros(3), distance=0.0,
               refit_normal=np.zeros(3), refit_distance=0.0, reference_point=np.zeros(3), margin=np.inf, first_sample=None)
    if n < 3:
        return res
    sampler = Sampler(n, seed)
    K = math.log(max(1 - confidence, 1.0e-5))
    iter_max, it = max_iterations, 0
    while it < iter_max:
        s = sampler.sample()
        if it == 0:
            res["first_sample"] = tuple(s)
        normal, distance = model(points[s[0]], points[s[1]], points[s[2]])
        e = errors(points, normal, distance)
        with np.errstate(invalid="ignore"):
            inl = e <= threshold
        if want_margin:
            gap = np.abs(e - threshold)
            gap = gap[np.isfinite(gap)]
            if len(gap):
                res["margin"] = min(res["margin"], float(gap.min()))
        good = int(inl.sum())
        if good > res["n_inliers"]:
            res.update(n_inliers=good, best_iteration=it, inlier_mask=inl.astype(np.uint8), normal=normal, distance=float(distance))
            den = math.log(1 - math.pow(good / float(n), 5)) if good < n else -math.inf
            if den != 0:
                N = K / den
                if N < iter_max:
                    iter_max = int(math.ceil(N)) if N > 0 else 0
        it += 1
    res["iterations"] = it
    count = res["n_inliers"]
    if count >= 3:
        p = points[res["inlier_mask"] == 1]
        cog = p.sum(0) / count
        d = p - cog
        cov = d.T @ d
        lam, vec = np.linalg.eigh(cov)
        v = orient(vec[:, 0] / np.linalg.norm(vec[:, 0]), res["normal"])
        tol_cog = 4 * count * EPS * np.abs(p).max()
        with np.errstate(divide="ignore"):
            tol_normal = 4 * count * EPS * np.trace(cov) / (lam[1] - lam[0]) + 16 * EPS
        tol_distance = np.linalg.norm(cog) * tol_normal + tol_cog + 4 * EPS * np.linalg.norm(cog)
        res.update(refit_valid=1, refit_normal=v, refit_distance=float(v @ cog), reference_point=cog, cov=cov, eigenvalues=lam, tol_cog=tol_cog,
                   tol_normal=tol_normal, tol_distance=tol_distance)
    return res


def margin(points, **kw):
    return reference(points, want_margin=True, **kw)["margin"]


# ---- point generator ----

def make_points(n, planes=((0.4, 0.01),), seed=1, extent=4.0, labels=False):
    """n points in a box of `extent` metres around (0, 0, 5); planes = ((fraction, noise), ...): that fraction of the points lies on a random plane
    through the box with Gaussian noise of that many metres along its normal.  The rest is uniform in the box.  The order is shuffled.
    labels=True: also the plane each point was put on (-1: none)."""
    rng = np.random.RandomState(seed)
    pts = rng.uniform(-extent / 2, extent / 2, (n, 3))
    which = np.full(n, -1)
    at = 0
    for number, (frac, noise) in enumerate(planes):
        k = int(round(frac * n))
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        u = np.cross(nrm, [1.0, 0.0, 0.0] if abs(nrm[0]) < 0.9 else [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        origin = rng.uniform(-extent / 8, extent / 8, 3)
        ab = rng.uniform(-extent / 2, extent / 2, (k, 2))
        pts[at:at + k] = origin + ab[:, :1] * u + ab[:, 1:] * v + rng.normal(0, noise, (k, 1)) * nrm if noise > 0 else origin + ab[:, :1] * u + ab[:, 1:] * v
        which[at:at + k] = number
        at += k
    order = rng.permutation(n)
    pts = np.ascontiguousarray(pts[order] + np.array([0.0, 0.0, 5.0]))
    return (pts, which[order]) if labels else pts


# ---- comparison ----

def ulp_diff(a, b):
    """largest distance in units in the last place between two float64 arrays of the same sign pattern (0 where the bits are equal)"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    ia, ib = a.view(np.int64), b.view(np.int64)
    return int(np.abs(ia - ib).max()) if len(ia) else 0


def compare(res, ref, strict, what=""):
    """the entry point's dict against reference()'s.  Returns the observed fractions of the refit tolerances."""
    assert res["n_inliers"] == ref["n_inliers"], (what, res["n_inliers"], ref["n_inliers"])
    assert res["iterations"] == ref["iterations"] and res["best_iteration"] == ref["best_iteration"], (what, res["iterations"], ref["iterations"], res["best_iteration"], ref["best_iteration"])
    assert (res["inlier_mask"] == ref["inlier_mask"]).all(), "%s: %d mask entries differ" % (what, (res["inlier_mask"] != ref["inlier_mask"]).sum())
    assert res["refit_valid"] == ref["refit_valid"]
    fig = dict(model_ulp=ulp_diff(np.append(res["normal"], res["distance"]), np.append(ref["normal"], ref["distance"])), cog=0.0, normal=0.0, distance=0.0)
    if strict:
        assert fig["model_ulp"] == 0, "%s: the RANSAC model differs from the restatement's bits by %d ulp" % (what, fig["model_ulp"])
    if ref["refit_valid"]:
        fig["cog"] = float(np.abs(res["reference_point"] - ref["reference_point"]).max() / ref["tol_cog"])
        fig["normal"] = float(np.linalg.norm(res["refit_normal"] - ref["refit_normal"]) / ref["tol_normal"])
        fig["distance"] = float(abs(res["refit_distance"] - ref["refit_distance"]) / ref["tol_distance"])
        print("%s: n_inliers %d iterations %d best %d; refit error / tolerance: cog %.3g normal %.3g distance %.3g (tol_normal %.3g)"
              % (what, res["n_inliers"], res["iterations"], res["best_iteration"], fig["cog"], fig["normal"], fig["distance"], ref["tol_normal"]))
        if strict or np.isfinite(ref["tol_normal"]):
            assert fig["cog"] <= 1.0 and fig["normal"] <= 1.0 and fig["distance"] <= 1.0, (what, fig)
        assert abs(np.linalg.norm(res["refit_normal"]) - 1.0) <= 4 * EPS
        assert res["refit_normal"] @ res["normal"] >= 0.0
    else:
        assert (res["refit_normal"] == 0).all() and res["refit_distance"] == 0 and (res["reference_point"] == 0).all()
    return fig


# ---- the host-only form (pvio_amd/host/plane_ransac.cpp) and the reference's own template, built into a directory of the caller's ----

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = "/root/reference"
GOLDEN = os.path.join(HERE, "golden", "plane_ransac_300.npz")
GOLDEN_CASE = dict(n=300, planes=((0.4, 0.01),), seed=1300)  # make_points arguments of the fixture: the reference's window, 40 % on a plane, 1 cm noise
CXXFLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]


def build_host_form(directory):
    """libplane_host.so = tests/host/plane_shim.cpp + pvio_amd/host/plane_ransac.cpp"""
    so = os.path.join(str(directory), "libplane_host.so")
    subprocess.check_call(["g++"] + CXXFLAGS + ["-fPIC", "-shared", "-w", "-o", so, os.path.join(HERE, "host", "plane_shim.cpp"),
                                                os.path.join(ROOT, "pvio_amd", "host", "plane_ransac.cpp")])
    return C.CDLL(so)


def host_form(lib, points, threshold=0.03, confidence=0.999, max_iterations=1000, seed=0):
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = len(points)
    mask, ints, d = np.zeros(max(n, 1), np.uint8), np.zeros(4, np.int32), np.zeros(11)
    f64p = C.POINTER(C.c_double)
    lib.host_plane_ransac(C.c_int(n), points.ctypes.data_as(f64p), C.c_double(threshold), C.c_double(confidence), C.c_int(max_iterations), C.c_uint32(seed),
                          mask.ctypes.data_as(C.POINTER(C.c_uint8)), ints.ctypes.data_as(C.POINTER(C.c_int32)), d.ctypes.data_as(f64p))
    return dict(n_inliers=int(ints[0]), iterations=int(ints[1]), best_iteration=int(ints[2]), refit_valid=int(ints[3]), inlier_mask=mask[:n], normal=d[0:3].copy(),
                distance=float(d[3]), refit_normal=d[4:7].copy(), refit_distance=float(d[7]), reference_point=d[8:11].copy())


def reference_available():
    return os.path.isfile(os.path.join(REFERENCE, "pvio", "src", "pvio", "utility", "ransac.h")) and shutil.which("g++") is not None


def build_ref_harness(directory):
    """tests/host/plane_ref_harness.cpp above the reference's headers, read in place; pvio/version.h generated as oracle/ref/Makefile generates it"""
    directory = str(directory)
    os.makedirs(os.path.join(directory, "gen", "pvio"), exist_ok=True)
    text = open(os.path.join(REFERENCE, "pvio", "cmake", "version.h.in")).read()
    for k, v in (("MAJOR", "0"), ("MINOR", "3"), ("PATCH", "0")):
        text = text.replace("${PROJECT_VERSION_%s}" % k, v)
    text = text.replace("#cmakedefine PVIO_ENABLE_THREADING", "/* #undef PVIO_ENABLE_THREADING */")
    for k in ("PVIO_DEBUG", "PVIO_ENABLE_FORENSICS", "PVIO_ENABLE_PLANE_CONSTRAINT"):
        text = text.replace("#cmakedefine %s" % k, "#define %s" % k)
    open(os.path.join(directory, "gen", "pvio", "version.h"), "w").write(text)
    exe = os.path.join(directory, "plane_ref_harness")
    subprocess.check_call(["g++"] + CXXFLAGS + ["-w", "-I" + os.path.join(directory, "gen"), "-I" + os.path.join(ROOT, "oracle", "ref", "eigen"),
                                                "-I" + os.path.join(REFERENCE, "pvio", "include"), "-I" + os.path.join(REFERENCE, "pvio", "src"), "-o", exe,
                                                os.path.join(HERE, "host", "plane_ref_harness.cpp")])
    return exe


def run_ref_harness(exe, points, threshold=0.03, confidence=0.999, max_iterations=1000, seed=0):
    """what the reference's own Ransac<3, PlaneState, PlaneSolver, PlaneEvaluator> returns: inlier_count, inlier_mask, normal, distance"""
    d = os.path.dirname(exe)
    np.ascontiguousarray(points, np.float64).tofile(os.path.join(d, "points.f64"))
    subprocess.check_call([exe, os.path.join(d, "points.f64"), os.path.join(d, "out.bin"), repr(float(threshold)), repr(float(confidence)), str(max_iterations), str(seed)])
    raw = open(os.path.join(d, "out.bin"), "rb").read()
    head = np.frombuffer(raw[:40], np.float64)
    return dict(inlier_count=int(head[0]), normal=head[1:4].copy(), distance=float(head[4]), inlier_mask=np.frombuffer(raw[40:], np.uint8).copy())


def golden_run(exe):
    points = make_points(**GOLDEN_CASE)
    par = dict(threshold=0.03, confidence=0.999, max_iterations=1000, seed=0)
    out = run_ref_harness(exe, points, **par)
    return dict(points=points, inlier_count=out["inlier_count"], inlier_mask=out["inlier_mask"], normal=out["normal"], distance=out["distance"], **par)


if __name__ == "__main__":  # python tests/plane_compare.py: (re)record tests/golden/plane_ransac_300.npz from the reference's own template
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        np.savez_compressed(GOLDEN, **golden_run(build_ref_harness(tmp)))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
