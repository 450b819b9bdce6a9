"""marginalize_frame parity: C-ABI (emulated build or GPU) vs the oracle.  The sqrt-information factor S is unique only
up to row order / sign (eigenvectors), so the comparison is made on the invariants S^T S, S^T s and on the Schur
complement (information matrix / vector) before the eigen-decomposition."""
import numpy as np

import ba_compare
from pvio_amd import BAState, BASummary


def solved_window(oracle, regular_prior=False, **kw):
    pb = ba_compare.make(oracle, **kw)
    if regular_prior:
        # a well-conditioned prior as produced by earlier marginalizations.  (With the first-time 1e15 gauge prior still
        # in the window -- information 1e30 -- eigenvalues below ~1e14 of the new prior are rounding noise in ANY
        # implementation, the reference's included; that case is only meaningful for victim 0, which removes it.)
        rng = np.random.default_rng(5)
        n = pb.prior_frames.shape[0]
        Q, _ = np.linalg.qr(rng.normal(size=(15 * n, 15 * n)))
        pb.prior_S = np.ascontiguousarray(np.diag(10.0 ** rng.uniform(0.5, 3.0, 15 * n)) @ Q)
        pb.prior_s = rng.normal(size=15 * n)
    st, sm = BAState(pb), BASummary(pb)
    oracle.solve(pb, st, sm)  # marginalization happens at a converged-ish state with non-zero residuals
    return pb, st


def set_regular_prior(pb, frames, seed=5):
    """solved_window's well-conditioned prior on any set of frames (none of them, all of them, not contiguous), linearized at the window's
    initial states"""
    frames = np.asarray(frames, np.int32)
    rng = np.random.default_rng(seed)
    n = frames.shape[0]
    Q, _ = np.linalg.qr(rng.normal(size=(15 * n, 15 * n)))
    pb.prior_frames = frames
    pb.prior_S = np.ascontiguousarray(np.diag(10.0 ** rng.uniform(0.5, 3.0, 15 * n)) @ Q)
    pb.prior_s = rng.normal(size=15 * n)
    pb.prior_lin_state = pb.frame_state[frames].copy()


def assert_finite_prior(S, s, IM, iv, what=""):
    """NaN / inf anywhere in the new prior fails loudly (an allclose with a tolerance scaled by a NaN maximum would not)"""
    for name, a in (("S", S), ("s", s), ("information matrix", IM), ("information vector", iv)):
        bad = ~np.isfinite(a)
        assert not bad.any(), "%s%s: %d non-finite entries, first at %s" % (what and what + ": ", name, int(bad.sum()), np.argwhere(bad)[0].tolist())


def check_marginalize(ctx, oracle, victim, pbst=None, expect=None, **kw):
    """`pbst`: a prepared (problem, state) instead of solved_window(**kw) (a test edits the window after the solve); `expect`: the
    oracle's (S, s, IM, iv) to compare with instead of oracle.marginalize on the same input (e.g. that of the window without a landmark)"""
    pb, st = pbst if pbst is not None else solved_window(oracle, regular_prior=(victim != 0), **kw)
    S0, s0, IM0, iv0 = expect if expect is not None else oracle.marginalize(pb, st, victim)
    S1, s1, IM1, iv1 = ctx.marginalize(pb, st, victim)
    assert_finite_prior(S0, s0, IM0, iv0, "oracle")
    assert_finite_prior(S1, s1, IM1, iv1, "kernels")
    scale = np.abs(IM0).max()
    np.testing.assert_allclose(IM1, IM0, rtol=1e-7, atol=1e-9 * scale)
    np.testing.assert_allclose(iv1, iv0, rtol=1e-7, atol=1e-9 * np.abs(iv0).max())
    assert np.abs(IM1 - IM1.T).max() <= 1e-9 * scale
    # S^T S reproduces the information matrix on its numerically non-null part; S^T s the information vector
    np.testing.assert_allclose(S1.T @ S1, S0.T @ S0, rtol=1e-6, atol=1e-7 * scale)
    np.testing.assert_allclose(S1.T @ s1, S0.T @ s0, rtol=1e-6, atol=1e-6 * np.abs(iv0).max())
    # spectrum: the part that is above the rounding noise of the matrix (eigenvalues within ~1e-12 of the largest are
    # noise: whether such a value falls on one or the other side of the reference's absolute 1e-8 cut depends on the
    # summation order and must not be compared) is reproduced by S^T S; everything else stays at noise level
    w = np.linalg.eigvalsh(IM1)
    keep = w > max(1e-8, 1e-11 * scale)
    wS = np.sort(np.linalg.eigvalsh(S1.T @ S1))
    np.testing.assert_allclose(wS[-keep.sum():], w[keep], rtol=1e-6)
    assert np.abs(wS[:len(wS) - keep.sum()]).max(initial=0.0) <= 1e-10 * scale
    # the new prior evaluated at its own linearization point has residual s (marginalization_error_cost.h:91):
    # cost there = |s|^2 / 2, gradient S^T s = projected information vector
    return dict(n=S1.shape[0], rank=int(keep.sum()))


def check_roles_agree(ctx1, ctx2, pb, st, victim, rtol=1e-9):
    """the register-tile landmark role (linearize_mode 1) against the large-window one (2) on the same input.  They evaluate the same
    factors and differ only in the order of the sums over landmarks / factors, so the information matrix and vector agree to rounding:
    rtol 1e-9 of each entry, with an absolute floor at 1e-9 of the largest entry (entries where the Schur complement cancels)."""
    S1, s1, IM1, iv1 = ctx1.marginalize(pb, st, victim)
    S2, s2, IM2, iv2 = ctx2.marginalize(pb, st, victim)
    assert_finite_prior(S1, s1, IM1, iv1, "first context")
    assert_finite_prior(S2, s2, IM2, iv2, "second context")
    scale = np.abs(IM1).max()
    np.testing.assert_allclose(IM2, IM1, rtol=rtol, atol=rtol * scale)
    np.testing.assert_allclose(iv2, iv1, rtol=rtol, atol=rtol * np.abs(iv1).max())
    return dict(info_matrix_rel=float(np.abs(IM2 - IM1).max() / scale), info_vector_rel=float(np.abs(iv2 - iv1).max() / np.abs(iv1).max()))


def sharded_window(oracle, spec):
    """the window of the sharded marginalization test (tests/test_multi_rank_cpu.py, multi_rank_worker.py): ba_compare.CASES[name] solved with
    a regular old prior; "name/by_anchor" lists its landmarks sorted by anchor frame (the reference's block order), so that contiguous landmark
    shards hold few anchors each and a rank can hold none of a victim's landmarks"""
    name, _, order = spec.partition("/")
    pb, st = solved_window(oracle, regular_prior=True, **ba_compare.CASES[name])
    if order == "by_anchor":
        from pvio_amd import synth
        keep = np.argsort(pb.lm_anchor_frame, kind="stable")
        pb2 = synth.permute_landmarks(pb, keep)
        st2 = BAState(pb2)
        st2.frame_state[:] = st.frame_state
        st2.lm_inv_depth = np.ascontiguousarray(st.lm_inv_depth[keep])
        return pb2, st2
    return pb, st
