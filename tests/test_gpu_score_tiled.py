"""The tiled importance + top-k kernels (score_tile_kernel + score_finish_kernel) on the device.  GPU box only (`-m gpu`).

Natural dispatch: shapes whose single-workgroup layout exceeds 160 KiB of LDS - refused before the tiled path existed - go through
ops.score_select / ops.importance unchanged.  Forced (rajni_debug_force_score_tiled): the small shapes at which tiling can go
wrong, N around the 32-token tile.  Scores are held to tests/numerics.py::importance_budget against the fp64 oracle; the
selection must be exactly the rule applied to the device's own scores.

N = 2 is the one size whose scores are not compared with the oracle: both centred rows have the same norm, the unbiased std is
0 up to rounding and z = (norm - mu) / 1e-6 amplifies the last bit of the norms into the whole range of the sigmoid (the
single-workgroup tests skip the comparison there too).  Everything else is checked at N = 2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_prefix as npx
import numerics_tiled as nt
from guarded import Guarded
from oracle import rajni_oracle as orc
from rajni_amd import _native as nat
from rajni_amd import ops

DEV = "cuda"
T = nt.TILE
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(nm.TORCH[dt])


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def plain_qkv(B, N, H, D, dt, seed=0):
    rng = np.random.default_rng([seed, B, N, H, D])
    return nm.round_to(rng.standard_normal((B, N, 3 * H * D), dtype=np.float32), dt)


def with_budget(key, make_qkv, H, dt):
    def make():
        q = make_qkv()
        return (q,) + nm.importance_budget(q, H, dt)
    return cached(key, make)


class forced_tiled:
    def __enter__(self):
        nat.lib().rajni_debug_force_score_tiled(1)

    def __exit__(self, *exc):
        nat.lib().rajni_debug_force_score_tiled(0)
        return False


def check_selection(s, idx, nxt, keep, P, what):
    """keep_idx exactly the rule on the device's own scores `s`, next_scores their gather"""
    sel = npx.select_tokens(s, keep, P)
    if P == 1:
        np.testing.assert_array_equal(sel, orc.select_tokens(s, keep), err_msg=what)
    np.testing.assert_array_equal(idx.cpu().numpy(), sel, err_msg=what)
    assert np.array_equal(host(nxt), np.take_along_axis(s, sel.astype(np.int64), axis=1), equal_nan=True), what


def keep_classes(n):
    return sorted({k for k in (1, n // 2, n - 1, n) if 1 <= k <= n})


# ---------------------------------------------------------------------------------------------------------------
# natural dispatch
# ---------------------------------------------------------------------------------------------------------------

NATURAL = [(2, 626, 2, 64, "bf16"), (1, 1374, 6, 64, "bf16"), (1, 1374, 6, 64, "fp16"), (1, 1025, 16, 64, "fp32"),
           (2, 577, 16, 80, "bf16"), (1, 320, 2, 128, "bf16"), (1, 4097, 2, 64, "bf16")]


@pytest.mark.parametrize("B,N,H,D,dt", NATURAL)
def test_long_shapes_take_the_tiled_path_by_themselves(B, N, H, D, dt):
    """no hook: each of these shapes was refused with the LDS error before"""
    assert nat.lib().rajni_score_select_workspace_bytes(B, N, H, D, nat.dtype_code(nm.TORCH[dt])) == nt.workspace_bytes(B, N, H, D)
    qkv, want, bud, e32 = with_budget(("nat", B, N, H, D, dt), lambda: plain_qkv(B, N, H, D, dt), H, dt)
    keep = orc.keep_count(0.7, N)
    x = dev(qkv, dt)
    scores, idx, nxt = ops.score_select(x, H, keep)
    alone = ops.importance(x, H)
    s = host(scores)
    nm.assert_within(s, want, bud, f"tiled importance {dt} {(B, N, H, D)} (e32 {e32:.2g})")
    assert torch.equal(alone.view(torch.uint8), scores.view(torch.uint8))
    check_selection(s, idx, nxt, keep, 1, f"tiled score_select {dt} {(B, N, H, D)}")
    none, idx2, nxt2 = ops.score_select(x, H, keep, want_scores=False)       # scores_out = NULL
    assert none is None and torch.equal(idx2, idx) and torch.equal(nxt2.view(torch.uint8), nxt.view(torch.uint8))
    # the entry points without scratch still refuse, with the LDS message
    with pytest.raises(NotImplementedError, match="LDS"):
        nat.check(nat.lib().rajni_importance(x.data_ptr(), alone.data_ptr(), B, N, H, D, 1e-6, nat.dtype_code(x.dtype),
                                             nat.stream_ptr(x.device)), "rajni_importance")


def test_natural_long_shape_with_prefix_tokens_and_every_keep_class():
    B, N, H, D, dt = 2, 626, 2, 64, "bf16"
    qkv, want, bud, _ = with_budget(("nat", B, N, H, D, dt), lambda: plain_qkv(B, N, H, D, dt), H, dt)
    x = dev(qkv, dt)
    first = None
    for P in (1, 5, 32):
        for keep in keep_classes(N - P):
            scores, idx, nxt = ops.score_select(x, H, keep, num_prefix=P)
            first = scores if first is None else first
            assert torch.equal(scores.view(torch.uint8), first.view(torch.uint8))       # the scores do not depend on P or keep
            check_selection(host(scores), idx, nxt, keep, P, f"natural P={P} keep={keep}")
    nm.assert_within(host(first), want, bud, "tiled importance bf16 (2, 626, 2, 64)")


# ---------------------------------------------------------------------------------------------------------------
# forced: sizes around the tile
# ---------------------------------------------------------------------------------------------------------------

SMALL_N = [2, T - 1, T, T + 1, 2 * T + 3, 197]
# H in {1, 3, 12} x D in {32, 64, 80, 128}, thinned: every head dim with two head counts, every head count with both lane mappings
HD = [(1, 32), (12, 32), (1, 64), (3, 64), (12, 64), (3, 80), (12, 80), (1, 128), (3, 128)]
HD_DT = [(h, d, dt) for i, (h, d) in enumerate(HD) for dt in (["bf16", "fp16", "fp32"] if (h, d) in ((3, 64), (3, 80)) else
                                                               [["bf16", "fp16", "fp32"][i % 3]])]


@pytest.mark.parametrize("H,D,dt", HD_DT)
@pytest.mark.parametrize("N", SMALL_N)
def test_forced_tiled_around_the_tile_size(N, H, D, dt):
    B = 3
    qkv, want, bud, e32 = with_budget(("small", B, N, H, D, dt), lambda: plain_qkv(B, N, H, D, dt, seed=1), H, dt)
    x = dev(qkv, dt)
    with forced_tiled():
        assert nat.lib().rajni_score_select_workspace_bytes(B, N, H, D, nat.dtype_code(x.dtype)) == nt.workspace_bytes(B, N, H, D)
        alone = ops.importance(x, H)
        s = host(alone)
        if N > 2:
            nm.assert_within(s, want, bud, f"forced tiled importance {dt} {(B, N, H, D)} (e32 {e32:.2g})")
        else:
            assert np.isfinite(s).all() and (s >= 0).all() and (s <= 1).all()
        for keep in keep_classes(N - 1):
            scores, idx, nxt = ops.score_select(x, H, keep)
            assert torch.equal(scores.view(torch.uint8), alone.view(torch.uint8))
            check_selection(s, idx, nxt, keep, 1, f"forced tiled {dt} {(B, N, H, D)} keep={keep}")
    if N > 2:   # the hook is off again: the single-workgroup kernel, inside the same budget (not the same bits: other sum orders)
        nm.assert_within(host(ops.importance(x, H)), want, bud, f"single-workgroup importance {dt} {(B, N, H, D)}")


@pytest.mark.parametrize("kind", nm.IMP_KINDS)
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("B,N,H,D", [(4, 197, 12, 64), (3, 61, 4, 80)])
def test_forced_tiled_stress_inputs(B, N, H, D, dt, kind):
    qkv, want, bud, e32 = with_budget(("imp", kind, B, N, H, D, dt), lambda: nm.importance_qkv(kind, B, N, H, D, dt), H, dt)
    keep = orc.keep_count(0.7, N)
    with forced_tiled():
        scores, idx, nxt = ops.score_select(dev(qkv, dt), H, keep)
        alone = ops.importance(dev(qkv, dt), H)
    s = host(scores)
    nm.assert_within(s, want, bud, f"forced tiled importance {kind} {dt} {(B, N, H, D)} (e32 {e32:.2g})")
    assert torch.equal(alone.view(torch.uint8), scores.view(torch.uint8))
    check_selection(s, idx, nxt, keep, 1, f"forced tiled {kind} {dt} {(B, N, H, D)}")


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("P,N,H,D", [(1, 2 * T + 3, 3, 64), (5, T + 1, 3, 80), (5, 197, 12, 64), (32, T + 1, 1, 32), (32, 2 * T + 3, 3, 128),
                                     (32, 33, 3, 64)])
def test_forced_tiled_prefix_tokens_and_keep_classes(P, N, H, D, dt):
    B = 2
    x = dev(plain_qkv(B, N, H, D, dt, seed=2), dt)
    with forced_tiled():
        alone = ops.importance(x, H)
        s = host(alone)
        for keep in keep_classes(N - P):
            scores, idx, nxt = ops.score_select(x, H, keep, num_prefix=P)
            assert tuple(idx.shape) == tuple(nxt.shape) == (B, P + keep)
            assert torch.equal(scores.view(torch.uint8), alone.view(torch.uint8))
            check_selection(s, idx, nxt, keep, P, f"forced tiled P={P} {dt} {(B, N, H, D)} keep={keep}")


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("N,H,D,forced", [(2 * T + 3, 3, 64, True), (197, 12, 80, True), (626, 2, 64, False)])
def test_ties_go_to_the_lower_index(N, H, D, dt, forced):
    """computed scores cannot be given special values, so ties are made by duplicating K and V rows: every patch token from row 6
    on repeats one of three rows (across tiles), its score must be bit-equal to its twins', and whatever the cut, the kept members
    of a class are its lowest indices"""
    B = 2
    qkv = plain_qkv(B, N, H, D, dt, seed=3).reshape(B, N, 3, H * D)
    src = 3 + (np.arange(6, N) % 3)
    qkv[:, 6:, 1:] = qkv[:, src, 1:]
    x = dev(qkv.reshape(B, N, -1), dt)
    hook = forced_tiled() if forced else None
    if hook:
        hook.__enter__()
    try:
        assert nat.lib().rajni_score_select_workspace_bytes(B, N, H, D, nat.dtype_code(x.dtype)) > 0
        s = host(ops.importance(x, H))
        for c in range(3):
            members = np.concatenate([[3 + c], 6 + np.nonzero(src == 3 + c)[0]])
            assert (s[:, members] == s[:, members[:1]]).all(), f"class {c}: twins' scores differ"
        for keep in (1, 2, 4, (N - 1) // 3, (N - 1) // 2, N - 3):
            scores, idx, nxt = ops.score_select(x, H, keep)
            check_selection(s, idx, nxt, keep, 1, f"ties N={N} keep={keep} {dt}")
            kept = idx.cpu().numpy()
            for b in range(B):
                for c in range(3):
                    members = np.concatenate([[3 + c], 6 + np.nonzero(src == 3 + c)[0]])
                    got = np.isin(members, kept[b])
                    assert not (np.diff(got.astype(int)) > 0).any(), f"a higher index of class {c} was kept over a lower one"
    finally:
        if hook:
            hook.__exit__()


# ---------------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("N,H,D,forced", [(2 * T + 3, 3, 64, True), (197, 4, 80, True), (626, 2, 64, False), (320, 2, 128, False)])
def test_same_bits_run_to_run_and_at_any_batch_position(N, H, D, dt, forced):
    B = 5
    x = dev(plain_qkv(B, N, H, D, dt, seed=4), dt)
    keep = orc.keep_count(0.6, N)
    hook = forced_tiled() if forced else None
    if hook:
        hook.__enter__()
    try:
        a = ops.score_select(x, H, keep)
        b = ops.score_select(x, H, keep)
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
        for i in range(B):
            one = ops.score_select(x[i:i + 1].contiguous(), H, keep)
            for u, v in zip(a, one):
                assert torch.equal(u[i:i + 1].contiguous().view(torch.uint8), v.view(torch.uint8)), f"image {i} alone differs"
    finally:
        if hook:
            hook.__exit__()


# ---------------------------------------------------------------------------------------------------------------
# poisoned buffers
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("B,P,N,H,D,forced", [(3, 5, 2 * T + 3, 3, 64, True), (2, 1, T + 1, 3, 80, True), (1, 5, 1374, 6, 64, False),
                                              (2, 1, 626, 2, 64, False)])
def test_guarded_outputs_and_workspace(B, P, N, H, D, dt, forced):
    """scores_out, keep_idx, next_scores and the scratch each sit in a poisoned arena: every output element written, both guards of
    every buffer intact (nothing is written past rajni_score_select_workspace_bytes), the Q third of tokens 1.. never read"""
    tdt = nm.TORCH[dt]
    code = nat.dtype_code(tdt)
    qkv = dev(plain_qkv(B, N, H, D, dt, seed=5), dt)
    qg = Guarded(tuple(qkv.shape), tdt, DEV).fill_(qkv)
    qg.arena[qg.offset:qg.end].view(B, N, -1)[:, 1:, : H * D * qg.esize] = 0xFF
    lib = nat.lib()
    lib.rajni_debug_force_score_tiled(int(forced))
    try:
        nbytes = lib.rajni_score_select_workspace_bytes(B, N, H, D, code)
        assert nbytes == nt.workspace_bytes(B, N, H, D)
        ref = None
        for keep in (0, 1, (N - P) // 2, N - P):
            what = f"score_select_ws B={B} P={P} N={N} H={H} D={D} keep={keep} {dt}"
            ws = Guarded((nbytes,), torch.uint8, DEV)
            sg = Guarded((B, N), tdt, DEV)
            ig = Guarded((B, P + keep), torch.int32, DEV) if keep else None
            ng = Guarded((B, P + keep), tdt, DEV) if keep else None
            nat.check(lib.rajni_score_select_ws(qg.ptr(), B, N, H, D, 1e-6, P, keep, sg.ptr(), ig.ptr() if keep else None,
                                                ng.ptr() if keep else None, code, ws.ptr(), nbytes, nat.stream_ptr()), "rajni_score_select_ws")
            torch.cuda.synchronize()
            ws.check(f"{what}: workspace", written=False)
            sg.check(f"{what}: scores")
            ref = sg.t.clone() if ref is None else ref
            assert torch.equal(sg.t.view(torch.uint8), ref.view(torch.uint8)), what
            if keep:
                ig.check(f"{what}: keep_idx")
                ng.check(f"{what}: next_scores")
                check_selection(host(sg.t), ig.t, ng.t, keep, P, what)
        qg.check("score_select_ws: qkv", written=False)
        s = host(ref)
        assert np.isfinite(s).all()
        want = orc.importance_scores(host(qkv), H)
        assert np.abs(s - want).max() <= (2e-5 if dt == "fp32" else 6e-3) * np.abs(want).max()
    finally:
        lib.rajni_debug_force_score_tiled(0)
