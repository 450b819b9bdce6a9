"""pvio_hip_triangulate against numpy: the reference, its tolerance and the checks that tests/test_triangulate.py runs in the emulator and on the GPU.

Reference: numpy.linalg.svd of the same 2K x 4 matrix (rows u P_2 - P_0, v P_2 - P_1), q = V^T[3] with the header's sign rule; gates, point and
score restated from geometry/stereo.h:104-128.  The kernel is a one-sided Jacobi on the rows, LAPACK's gesdd a bidiagonalization: two algorithms.

Tolerance of a track, from the reference alone:
  bound   = 8 K eps sigma_1 / (sigma_3 - sigma_4), eps = 2^-52: rows x columns x the normwise perturbation bound of a singular vector
  spread  = the largest change of the reference's q over 8 copies of the input (view_P, obs_z) with every entry moved by one ulp up or down
  tol_q   = max(bound, 4 spread)           (4: the factor ba_compare.py uses for the oracle's own reordering spread)
  tol_point = tol_q (|q_3| + |q[0..2]|) / q_3^2           for a track that is ok: the first-order change of q[0..2] / q_3
            = 2 tol_q / |q[0..2]|                            for one that is not: the change of q[0..2] / |q[0..2]| is at most that of q[0..2] over
                                                             the length, once for the numerator and once for the length itself
  tol_score = (2 / K) sum_i |e_i| d_i + (1 / K) sum_i d_i^2 + 16 eps (score + mean |z_i|^2),   d_i = 2 |J_i|_F |P_i|_F tol_q
              e_i the reprojection term, J_i the Jacobian of y -> y[0..1] / y[2] at the reference's y_i: the first-order change of the sum of
              squares (the 2 covers the second order), plus the rounding of evaluating it
A strict case also asserts tol_q <= 1e-9.  `ok` must be identical for every track, and the reference itself must sit away from the gates:
|y_i[2] q_3| >= 1e-6 |y_i| and |100 - y_i[2] / q_3| >= 1e-6 * 100 for every observation."""
import numpy as np

from pvio_amd import synth

EPS = 2.0 ** -52
MAX_OBS = 32      # PVIO_TRI_MAX_OBS
MAX_SWEEPS = 30   # kTriMaxSweeps of pvio_amd/csrc/ba_triangulate.h
GATE_MARGIN = 1e-6


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------

def arc_views(n=MAX_OBS, kf_dt=0.25):
    """(view_P [n, 3, 4], R_wc, p_wc) of synth's orbit with synth's camera extrinsic"""
    R_bc = synth.qmat(synth.Q_BC / np.linalg.norm(synth.Q_BC))
    R_wc, p_wc = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for i in range(n):
        R, p, _, _ = synth._pose(i * kf_dt)
        R_wc[i], p_wc[i] = R @ R_bc, p + R @ synth.P_BC
    return views_from_poses(R_wc, p_wc), R_wc, p_wc


def views_from_poses(R_wc, p_wc):
    P = np.zeros((R_wc.shape[0], 3, 4))
    P[:, :, :3] = np.transpose(R_wc, (0, 2, 1))
    P[:, :, 3] = -np.einsum("nji,nj->ni", R_wc, p_wc)
    return P


def project(view_P, views, point):
    y = view_P[views] @ np.append(point, 1.0)
    return y[:, :2] / y[:, 2:3], y[:, 2]


def make_tracks(Ks, seed, noise=True, depth=(2.0, 8.0), descending=False):
    """One track per entry of Ks over synth's arc: K consecutive views from a random start, a point whose depth is inside `depth` in every one of
    them and that projects inside the image, observations with synth's pixel noise.  Returns a dict with the CSR input and the true points."""
    view_P, _, _ = arc_views()
    rng = synth.Rng(seed)
    sigma = np.sqrt(synth.KEYPOINT_COV) / synth.K_EUROC[:2]  # pixels -> normalized coordinates
    ptr, obs_view, obs_z, truth = [0], [], [], []
    for K in Ks:
        start = int(rng.uniform(1)[0] * (MAX_OBS - K + 1))
        views = np.arange(start, start + K)
        while True:
            u = rng.uniform(3)
            cand = np.array([(u[0] - 0.5) * 5.0, (u[1] - 0.5) * 5.0, (u[2] - 0.5) * 2.4])
            z, d = project(view_P, views, cand)
            if (d > depth[0]).all() and (d < depth[1]).all() and (np.abs(z[:, 0]) < 0.7).all() and (np.abs(z[:, 1]) < 0.45).all():
                break
        if noise:
            z = z + rng.normal(2 * K).reshape(K, 2) * sigma
        order = np.arange(K)[::-1] if descending else np.arange(K)
        obs_view.extend(views[order]), obs_z.extend(z[order]), truth.append(cand)
        ptr.append(len(obs_view))
    return dict(view_P=view_P, track_ptr=np.array(ptr, np.int32), obs_view=np.array(obs_view, np.int32),
                obs_z=np.array(obs_z, float).reshape(-1, 2), truth=np.array(truth, float).reshape(-1, 3))


def reversed_inside_tracks(inp):
    """the same tracks with the observations of each in the opposite order"""
    idx = np.concatenate([np.arange(a, b)[::-1] for a, b in zip(inp["track_ptr"][:-1], inp["track_ptr"][1:])]) if len(inp["obs_view"]) else np.zeros(0, int)
    return dict(inp, obs_view=np.ascontiguousarray(inp["obs_view"][idx]), obs_z=np.ascontiguousarray(inp["obs_z"][idx]))


# ---- reference ---------------------------------------------------------------------------------------------------------------------------------

def _systems(P, z):
    """P [T, K, 3, 4], z [T, K, 2] -> A [T, 2K, 4]"""
    T, K = z.shape[:2]
    A = np.zeros((T, 2 * K, 4))
    A[:, 0::2] = z[:, :, 0:1] * P[:, :, 2] - P[:, :, 0]
    A[:, 1::2] = z[:, :, 1:2] * P[:, :, 2] - P[:, :, 1]
    return A


def _null_vectors(A):
    _, s, Vt = np.linalg.svd(A)
    q = Vt[:, 3].copy()
    # q_3 >= 0; if q_3 == 0 the first non-zero of q[0..2] is positive
    key = np.where(q[:, 3] != 0, q[:, 3], np.where(q[:, 0] != 0, q[:, 0], np.where(q[:, 1] != 0, q[:, 1], q[:, 2])))
    q[key < 0] *= -1.0
    return q, s


def _reference_same_K(P, z):
    T, K = z.shape[:2]
    finite = np.isfinite(z).all((1, 2)) & np.isfinite(P).all((1, 2, 3))
    Pf, zf = np.where(finite[:, None, None, None], P, 0.0), np.where(finite[:, None, None], z, 0.0)
    q, s = _null_vectors(_systems(Pf, zf))
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = 8 * K * EPS * s[:, 0] / (s[:, 2] - s[:, 3])
        rng = np.random.RandomState(12345)
        spread = np.zeros(T)
        for _ in range(8):
            Pp = np.nextafter(Pf, np.where(rng.rand(*Pf.shape) < 0.5, -np.inf, np.inf))
            zp = np.nextafter(zf, np.where(rng.rand(*zf.shape) < 0.5, -np.inf, np.inf))
            qp, _ = _null_vectors(_systems(Pp, zp))
            spread = np.maximum(spread, np.linalg.norm(qp - q, axis=1))
        tol_q = np.maximum(bound, 4 * spread)
        y = np.einsum("tkij,tj->tki", Pf, q)
        q3 = q[:, 3:4]
        ok = ((y[:, :, 2] * q3 > 0) & (y[:, :, 2] / q3 < 100)).all(1)
        margin = np.minimum(np.abs(y[:, :, 2] * q3) / np.linalg.norm(y, axis=2), np.abs(100 - y[:, :, 2] / q3) / 100).min(1)
        len3 = np.linalg.norm(q[:, :3], axis=1)
        point = np.where(ok[:, None], q[:, :3] / q3, q[:, :3] / np.where(len3 > 0, len3, 1.0)[:, None])
        tol_point = np.where(ok, tol_q * (np.abs(q[:, 3]) + len3) / q[:, 3] ** 2, 2 * tol_q / len3)
        e = y[:, :, :2] / y[:, :, 2:3] - zf
        score = (e ** 2).sum((1, 2)) / K
        y2 = y[:, :, 2]
        J_F = np.sqrt(2 / y2 ** 2 + (y[:, :, 0] ** 2 + y[:, :, 1] ** 2) / y2 ** 4)
        d = 2 * J_F * np.linalg.norm(Pf, axis=(2, 3)) * tol_q[:, None]
        tol_score = (2 * np.linalg.norm(e, axis=2) * d + d ** 2).sum(1) / K + 16 * EPS * (score + (zf ** 2).sum((1, 2)) / K)
    nan = ~finite
    ok[nan], margin[nan] = False, np.inf  # the negated comparisons: a NaN fails the gates, and it is not near them
    return dict(q=q, sigma=s, bound=bound, spread=spread, tol_q=tol_q, ok=ok.astype(np.uint8), margin=margin, point=point, tol_point=tol_point,
                score=score, tol_score=tol_score, finite=finite)


def reference(view_P, track_ptr, obs_view, obs_z):
    """every track of the call; tracks with fewer than 2 observations get the header's values and tol 0"""
    view_P = np.asarray(view_P, float).reshape(-1, 3, 4)
    T = len(track_ptr) - 1
    Ks = np.diff(track_ptr)
    out = dict(q=np.zeros((T, 4)), sigma=np.zeros((T, 4)), bound=np.zeros(T), spread=np.zeros(T), tol_q=np.zeros(T), ok=np.zeros(T, np.uint8),
               margin=np.full(T, np.inf), point=np.zeros((T, 3)), tol_point=np.zeros(T), score=np.full(T, np.inf), tol_score=np.zeros(T),
               finite=np.ones(T, bool), K=Ks)
    for K in sorted(set(Ks.tolist())):
        if K < 2:
            continue
        sel = np.flatnonzero(Ks == K)
        idx = track_ptr[sel][:, None] + np.arange(K)[None, :]
        r = _reference_same_K(view_P[obs_view[idx]], obs_z[idx])
        for k, v in r.items():
            out[k][sel] = v
    return out


# ---- checks ------------------------------------------------------------------------------------------------------------------------------------

def call(ctx, inp):
    return ctx.triangulate(inp["view_P"], inp["track_ptr"], inp["obs_view"], inp["obs_z"], homogeneous=True)


def compare(res, ref, strict=True, what=""):
    """every track of a result against the reference.  Returns the figures of the case (printed by the tests, written down by prof_triangulate.py)"""
    T = len(ref["K"])
    short, nan = ref["K"] < 2, ~ref["finite"]
    cmp_ = ~short & ~nan
    assert (ref["margin"][cmp_] >= GATE_MARGIN).all(), "%s: the reference itself sits at a gate: margin %.3g" % (what, ref["margin"][cmp_].min())
    assert (res["ok"] == ref["ok"]).all(), "%s: ok differs at tracks %s" % (what, np.flatnonzero(res["ok"] != ref["ok"])[:8])
    # tracks with fewer than 2 observations: the header's values, exactly
    assert (res["ok"][short] == 0).all() and (res["point"][short] == 0).all() and (res["homogeneous"][short] == 0).all()
    assert (res["score"][short] == np.inf).all()
    assert (res["ok"][nan] == 0).all()
    if strict:
        assert (ref["tol_q"][cmp_] <= 1e-9).all(), "%s: tol_q %.3g" % (what, ref["tol_q"][cmp_].max())
    q = res["homogeneous"]
    assert np.allclose(np.linalg.norm(q[cmp_], axis=1), 1.0, rtol=0, atol=16 * EPS)
    assert (q[cmp_, 3] >= 0).all()
    e_q = np.linalg.norm(q - ref["q"], axis=1)
    e_p = np.linalg.norm(res["point"] - ref["point"], axis=1)
    with np.errstate(invalid="ignore"):
        e_s = np.abs(res["score"] - ref["score"])
    fig = dict(tracks=T, worst_q=0.0, worst_point=0.0, worst_score=0.0, tol_q_max=0.0)
    if cmp_.any():
        with np.errstate(divide="ignore", invalid="ignore"):  # (the tracks outside cmp_ have tol 0)
            ratio_q, ratio_p, ratio_s = e_q / ref["tol_q"], e_p / ref["tol_point"], e_s / ref["tol_score"]
        fig.update(worst_q=float(ratio_q[cmp_].max()), worst_point=float(ratio_p[cmp_].max()), worst_score=float(ratio_s[cmp_].max()), tol_q_max=float(ref["tol_q"][cmp_].max()), tol_q_min=float(ref["tol_q"][cmp_].min()))
    print(what, fig)
    bad = cmp_ & ~(e_q <= ref["tol_q"])
    assert not bad.any(), "%s: |q - q_ref| %s > tol_q %s at tracks %s" % (what, e_q[bad][:4], ref["tol_q"][bad][:4], np.flatnonzero(bad)[:4])
    bad = cmp_ & ~(e_p <= ref["tol_point"])
    assert not bad.any(), "%s: |point - point_ref| %s > tol_point %s at tracks %s" % (what, e_p[bad][:4], ref["tol_point"][bad][:4], np.flatnonzero(bad)[:4])
    bad = cmp_ & ~(e_s <= ref["tol_score"])
    assert not bad.any(), "%s: |score - score_ref| %s > tol_score %s at tracks %s" % (what, e_s[bad][:4], ref["tol_score"][bad][:4], np.flatnonzero(bad)[:4])
    return fig


def check(ctx, inp, ref=None, strict=True, what=""):
    ref = ref if ref is not None else reference(inp["view_P"], inp["track_ptr"], inp["obs_view"], inp["obs_z"])
    res = call(ctx, inp)
    fig = compare(res, ref, strict=strict, what=what)
    fig["max_sweeps"] = ctx.triangulate_stats()[0]
    return res, fig
