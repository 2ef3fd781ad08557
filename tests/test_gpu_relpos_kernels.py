"""The kernels of include/rajni_hip_relpos.h through the C ABI into guarded buffers: attention with a relative position bias in
every form a head-dim-64 shape is dispatched to, bf16 / fp16 / fp32 (rajni_debug_force_attention 0 and 2 both give the one-shot
kernel - a bias launch never takes the persistent one - so the budgets run under 0 and 1 and one test holds 2 to 0's bits), and score-select
with the class row's bias on the one-workgroup and the tiled path.  Budgets: tests/numerics_relpos.py.  GPU box only (`-m gpu`)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_prefix as npx
import numerics_relpos as nrp
from guarded import Guarded
from oracle import rajni_oracle as orc
from rajni_amd import ops, _native as nat

DEV = "cuda"
B, H, D = 2, 2, 64
SCALE = D ** -0.5
MODES = {0: "one_shot", 1: "online_chunked"}
# (name, gh, gw, P, Np or None = unpruned)
SHAPES = [
    ("n16_3x5", 3, 5, 1, None),            # the smallest case
    ("np33_4x8", 4, 8, 1, None),           # one key into a second 32-key block
    ("197_14x14", 14, 14, 1, None),        # the full square grid
    ("197to99", 14, 14, 1, 99),            # positions not contiguous
    ("257_16x16", 16, 16, 1, None),        # the chunked kernel
    ("257to130", 16, 16, 1, 130),          # a pruned chunked-size grid
    ("n22_3x7", 3, 7, 1, None),            # axis order
]
KINDS = ("peaked", "negative", "uniform")
_cache = {}


def cached(key, make):
    if key not in _cache:
        if len(_cache) >= 3:
            _cache.pop(next(iter(_cache)))
        _cache[key] = make()
    return _cache[key]


def tdt(dt):
    return nm.TORCH[dt]


def guarded_in(a, dtype, **kw):
    a = np.ascontiguousarray(a)
    g = Guarded(a.shape, dtype, device=DEV, **kw)
    g.fill_(torch.from_numpy(a.astype(np.float32) if dtype.is_floating_point else a.astype(np.int32)))
    return g


def reference(name, gh, gw, P, Np, dt, kind, tkind, b=B, h=H):
    def make():
        N = gh * gw + P
        np_ = N if Np is None else Np
        qkv = nm.attention_qkv(kind, b, N, h, D, dt)
        pos = nrp.kept_positions(np.random.default_rng([N, np_]), b, N, np_, P)
        g = qkv if Np is None else orc.gather_rows(qkv, pos.astype(np.int64))
        tab = nrp.kernel_tables(tkind, h, gh, gw)
        bias = nrp.batch_bias(*tab, gh, gw, P, pos)
        return (qkv, pos, tab) + nrp.attention_budget(g, h, SCALE, dt, bias)
    return cached((name, dt, kind, tkind, b, h), make)


def run_attention(qkv, pos, tab, gh, gw, P, dt, h=H, pruned=True, relpos=True):
    """rajni_attention_relpos (or rajni_attention) on guarded buffers; returns the fp64 output after the guard checks"""
    b, N = qkv.shape[:2]
    np_ = pos.shape[1]
    gq = guarded_in(qkv, tdt(dt))
    gidx = guarded_in(pos, torch.int32, fill_int32=0) if pruned else None
    gpos = guarded_in(pos, torch.int32, fill_int32=0) if pruned else None
    gt, gpq, gpk, gpqk = (guarded_in(a, torch.float32) for a in tab)
    out = Guarded((b, np_, h * D), tdt(dt), device=DEV)
    s = nat.stream_ptr(torch.device(DEV))
    if relpos:
        nat.check(nat.lib().rajni_attention_relpos(gq.ptr(), gidx.ptr() if pruned else None, out.ptr(), b, N, np_, h, D, SCALE,
                                                   nat.dtype_code(tdt(dt)), gt.ptr(), gpq.ptr(), gpk.ptr(), gpqk.ptr(), gh, gw, P,
                                                   gpos.ptr() if pruned else None, s), "rajni_attention_relpos")
    else:
        nat.check(nat.lib().rajni_attention(gq.ptr(), gidx.ptr() if pruned else None, out.ptr(), b, N, np_, h, D, SCALE,
                                            nat.dtype_code(tdt(dt)), s), "rajni_attention")
    torch.cuda.synchronize()
    out.check("attention output")
    for g in (gq, gt, gpq, gpk, gpqk) + ((gidx, gpos) if pruned else ()):
        g.check("attention input", written=False)
    return out.t.float().cpu().numpy().astype(np.float64), out.t.clone()


ATTN_CASES = [pytest.param(*shape, dt, kind, tkind, mode, id=f"{shape[0]}-{dt}-{kind}-{tkind}-{MODES[mode]}")
              for shape in SHAPES for dt in ("bf16", "fp16", "fp32") for kind in KINDS for tkind in nrp.TABLE_KINDS
              for mode in ((0,) if dt == "fp32" or (shape[4] or shape[1] * shape[2] + shape[3]) > 256 else (0, 1))]


@pytest.mark.parametrize("name,gh,gw,P,Np,dt,kind,tkind,mode", ATTN_CASES)
def test_attention_relpos_budget(name, gh, gw, P, Np, dt, kind, tkind, mode):
    qkv, pos, tab, want, bud = reference(name, gh, gw, P, Np, dt, kind, tkind)
    nat.lib().rajni_debug_force_attention(mode)
    try:
        got, _ = run_attention(qkv, pos, tab, gh, gw, P, dt, pruned=Np is not None)
    finally:
        nat.lib().rajni_debug_force_attention(0)
    nm.assert_within(got, want, bud, f"attention relpos {name} {kind} {tkind} {dt} mode {mode}")


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_attention_relpos_at_the_cap(dt):
    """32 x 32 + 1 tokens, once per kernel family: the cap's table size (63 * 63 entries per head), one image"""
    qkv, pos, tab, want, bud = reference("cap_32x32", 32, 32, 1, None, dt, "peaked", "normal", b=1)
    got, _ = run_attention(qkv, pos, tab, 32, 32, 1, dt, pruned=False)
    nm.assert_within(got, want, bud, f"attention relpos 32x32 {dt}")


@pytest.mark.parametrize("dt,mode", [(dt, mode) for dt in ("bf16", "fp16", "fp32") for mode in ((0,) if dt == "fp32" else (0, 1))])
@pytest.mark.parametrize("name,gh,gw,P,Np", [s for s in SHAPES if s[0] in ("np33_4x8", "197to99", "257to130", "257_16x16")])
def test_zero_tables_reproduce_rajni_attention_bit_for_bit(name, gh, gw, P, Np, dt, mode):
    qkv, pos, _, _, _ = reference(name, gh, gw, P, Np, dt, "peaked", "normal")
    zero = tuple(np.zeros_like(a) for a in nrp.kernel_tables("normal", H, gh, gw))
    nat.lib().rajni_debug_force_attention(mode)
    try:
        _, a = run_attention(qkv, pos, zero, gh, gw, P, dt, pruned=Np is not None)
        _, b = run_attention(qkv, pos, zero, gh, gw, P, dt, pruned=Np is not None, relpos=False)
    finally:
        nat.lib().rajni_debug_force_attention(0)
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_ops_attention_and_the_forced_full_row_mode_give_the_c_abi_bits(dt):
    """ops.attention(rel_pos=, pos=) is rajni_attention_relpos, and rajni_debug_force_attention(2) launches what 0 launches"""
    name, gh, gw, P, Np = SHAPES[3]
    qkv, pos, tab, _, _ = reference(name, gh, gw, P, Np, dt, "peaked", "normal")
    _, want = run_attention(qkv, pos, tab, gh, gw, P, dt)
    idx = torch.from_numpy(pos.astype(np.int32)).to(DEV)
    rp = ops.RelPos(*(torch.from_numpy(a).to(DEV) for a in tab), (gh, gw))
    q = torch.from_numpy(qkv).to(DEV).to(tdt(dt))
    got = ops.attention(q, idx, H, SCALE, rel_pos=rp, pos=idx, num_prefix=P)
    assert got.dtype == want.dtype and torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    nat.lib().rajni_debug_force_attention(2)
    try:
        _, full = run_attention(qkv, pos, tab, gh, gw, P, dt)
    finally:
        nat.lib().rajni_debug_force_attention(0)
    assert torch.equal(full.view(torch.uint8), want.view(torch.uint8))
    with pytest.raises(ValueError, match="pos without rel_pos"):
        ops.attention(q, idx, H, SCALE, pos=idx)


def test_refusals_of_the_attention_entry():
    q = torch.zeros(1, 17, 3 * 64, dtype=torch.bfloat16, device=DEV)
    z = torch.zeros(2 * 63 * 63 + 8, dtype=torch.float32, device=DEV)
    s = nat.stream_ptr(torch.device(DEV))
    out = torch.empty(1, 17, 64, dtype=torch.bfloat16, device=DEV)

    def call(Dh=64, gh=4, gw=4):
        return nat.lib().rajni_attention_relpos(q.data_ptr(), None, out.data_ptr(), 1, 17, 17, 64 // Dh, Dh, 0.125, nat.RAJNI_BF16,
                                                z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), gh, gw, 1, None, s)
    assert call() == 0
    assert call(Dh=32) == 2 and b"head dim 64 only" in nat.lib().rajni_last_error()
    assert call(gh=33, gw=1) == 2 and b"at most 32 x 32" in nat.lib().rajni_last_error()


# ---------------------------------------------------------------------------------------------------------------
# score-select with the class row's bias
# ---------------------------------------------------------------------------------------------------------------
SCORE_SHAPES = [(16, 1), (33, 1), (197, 1), (257, 3)]        # (N, P)


@pytest.mark.parametrize("tiled", [0, 1], ids=["one_workgroup", "tiled"])
@pytest.mark.parametrize("kind", ["peaked", "negative", "voffset"])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("N,P", SCORE_SHAPES)
def test_score_select_relpos_budget(N, P, dt, kind, tiled):
    def make():
        qkv = nm.importance_qkv(kind, B, N, H, D, dt)
        _, pq, _, pqk = nrp.kernel_tables("normal", H, 2, 2, seed=N)
        return (qkv, pq, pqk) + nrp.importance_budget(qkv, H, dt, pq, pqk, P)
    qkv, pq, pqk, want, bud, e32 = cached(("imp", N, P, dt, kind), make)
    keep = npx.keep_count(0.7, N, P)
    nat.lib().rajni_debug_force_score_tiled(tiled)
    try:
        nbytes = nat.lib().rajni_score_select_workspace_bytes(B, N, H, D, nat.dtype_code(tdt(dt)))
        assert (nbytes > 0) == bool(tiled)
        gq = guarded_in(qkv, tdt(dt))
        gpq, gpqk = guarded_in(pq, torch.float32), guarded_in(pqk, torch.float32)
        sc, nx = Guarded((B, N), tdt(dt), device=DEV), Guarded((B, P + keep), tdt(dt), device=DEV)
        ix = Guarded((B, P + keep), torch.int32, device=DEV)
        alone = Guarded((B, N), tdt(dt), device=DEV)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
        s = nat.stream_ptr(torch.device(DEV))
        for k, so, io, no in ((keep, sc, ix, nx), (0, alone, None, None)):       # with the selection, and the importance-only form
            nat.check(nat.lib().rajni_score_select_relpos(gq.ptr(), B, N, H, D, 1e-6, P, k, so.ptr(), io.ptr() if io else None,
                                                          no.ptr() if no else None, nat.dtype_code(tdt(dt)),
                                                          ws.data_ptr() if nbytes else None, nbytes, gpq.ptr(), gpqk.ptr(), s),
                      "rajni_score_select_relpos")
        torch.cuda.synchronize()
    finally:
        nat.lib().rajni_debug_force_score_tiled(0)
    for g in (sc, nx, ix, alone):
        g.check("score output")
    for g in (gq, gpq, gpqk):
        g.check("score input", written=False)
    got = sc.t.float().cpu().numpy().astype(np.float64)
    nm.assert_within(got, want, bud, f"score relpos {kind} {dt} N={N} P={P} {'tiled' if tiled else 'one workgroup'} (e32 {e32:.2g})")
    assert torch.equal(alone.t, sc.t)
    idx = ix.t.cpu().numpy()
    np.testing.assert_array_equal(idx, npx.select_tokens(got, keep, P))           # the rule on the device's own scores
    np.testing.assert_array_equal(nx.t.float().cpu().numpy().astype(np.float64), np.take_along_axis(got, idx.astype(np.int64), axis=1))


@pytest.mark.parametrize("tiled", [0, 1], ids=["one_workgroup", "tiled"])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_zero_values_reproduce_score_select_ws_bit_for_bit(dt, tiled):
    N, P = 197, 1
    keep = npx.keep_count(0.7, N, P)
    q = torch.from_numpy(nm.importance_qkv("peaked", B, N, H, D, dt)).to(DEV).to(tdt(dt))
    zero = ops.RelPos(torch.zeros(H, 9, device=DEV), *(torch.zeros(H, device=DEV) for _ in range(3)), (2, 2))
    nat.lib().rajni_debug_force_score_tiled(tiled)
    try:
        a = ops.score_select(q, H, keep, num_prefix=P, rel_pos=zero)
        b = ops.score_select(q, H, keep, num_prefix=P)
    finally:
        nat.lib().rajni_debug_force_score_tiled(0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
