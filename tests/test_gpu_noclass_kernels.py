"""rajni_score_select_query (include/rajni_hip_query.h) on the device: the mean importance query and selection with P = 0, in
the one-workgroup kernel (both LDS layouts) and on the tiled path, against tests/numerics_noclass.py.  GPU box only (`-m gpu`).

Scores are held element by element to numerics_noclass.importance_budget (numerics.importance_budget's (u_out + 4 e32) |want|
+ floor, e32 from the restatement's fp32 run, plus the derived worst case of another summation order of the mean) and, because
that e32 is one number per tensor and is 1 wherever a score leaves the fp32 range, the scores above 2^-80 to the same form with e32
taken over them alone (numerics_noclass.importance_budget_normal_range); selection is bit-exact against numerics_prefix.select_tokens on the device's own scores, the project's way of separating ranking from
scoring."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_noclass as nq
import numerics_prefix as npx
from guarded import Guarded
from rajni_amd import _native as nat
from rajni_amd import ops
from rajni_amd.wrapper.importance import compute_importance_query

DEV = "cuda"
KINDS = nm.IMP_KINDS + nq.QUERY_KINDS
# (B, N, H, D, P, keeps): the smallest sequence; a tile edge (tiles are 32 tokens); a tile edge with registers; head dim 80
# (the general lane mapping); ViT-B's token count (7 tiles); head dim 128
SHAPES = [(3, 5, 1, 8, 0, (1, 5)), (3, 33, 2, 64, 0, (16,)), (3, 65, 2, 64, 4, (30,)), (3, 50, 2, 80, 1, (24,)),
          (3, 197, 3, 64, 0, (147,)), (3, 130, 2, 128, 0, (65,))]
IDS = [f"N{s[1]}H{s[2]}D{s[3]}P{s[4]}" for s in SHAPES]


def lib():
    return nat.lib()


def stream():
    return nat.stream_ptr(torch.device(DEV))


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(nm.TORCH[dt])


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def run_query(qkv, H, P, keep, query, want_scores=True):
    """(scores, keep_idx, next_scores) of rajni_score_select_query with scratch of its own size query"""
    B, N, threeC = qkv.shape
    D = threeC // 3 // H
    code = nat.dtype_code(qkv.dtype)
    nbytes = lib().rajni_score_select_query_workspace_bytes(B, N, H, D, code, query)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes else None
    scores = torch.empty((B, N), dtype=qkv.dtype, device=DEV) if want_scores else None
    idx = torch.empty((B, P + keep), dtype=torch.int32, device=DEV) if keep else None
    nxt = torch.empty((B, P + keep), dtype=qkv.dtype, device=DEV) if keep else None
    nat.check(lib().rajni_score_select_query(qkv.data_ptr(), B, N, H, D, 1e-6, P, keep, query, nat.ptr(scores), nat.ptr(idx),
                                             nat.ptr(nxt), code, nat.ptr(ws), nbytes, stream()), "rajni_score_select_query")
    torch.cuda.synchronize()
    return scores, idx, nxt, nbytes


def bits(t):
    return t.contiguous().view(torch.uint8)


def check_selection(scores, idx, nxt, keep, P, what):
    s = scores.float().cpu().numpy()
    sel = npx.select_tokens(s, keep, P)
    np.testing.assert_array_equal(idx.cpu().numpy(), sel, err_msg=what)
    assert np.array_equal(nxt.float().cpu().numpy(), np.take_along_axis(s, sel, axis=1), equal_nan=True), what


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,H,D,P,keeps", SHAPES, ids=IDS)
def test_mean_query_scores_and_selection(B, N, H, D, P, keeps, kind, dt):
    make = nq.query_qkv if kind in nq.QUERY_KINDS else nm.importance_qkv
    qkv = make(kind, B, N, H, D, dt)
    want, bud, e32 = nq.importance_budget(qkv, H, dt)
    mask, bud_n, e32n = nq.importance_budget_normal_range(qkv, H, dt)      # (the scores an fp32 run can hold: see its docstring)
    q = dev(qkv, dt)
    what = f"mean query {kind} N={N} H={H} D={D} P={P} {dt}"

    def within(got, where):
        nm.assert_within(host(got), want, bud, f"{what}, {where}")
        r, _ = nm.worst_ratio(host(got)[mask], want[mask], bud_n[mask])
        print(f"[noclass] {what}, {where}: scores >= 2^-80 ({int(mask.sum())} of {mask.size}) worst err/budget {r:.3f} (e32 {e32n:.3g})")
        assert r <= 1.0, f"{what}, {where}: a score in the fp32 range is {r:.3g} x its budget off"
    try:
        # ---- one workgroup: the merged layout and the two-pass one give the same bits
        ref, _, _, nbytes = run_query(q, H, P, 0, nat.QUERY_MEAN)
        assert nbytes == 0
        print(f"[noclass] {what}: e32 {e32:.3g}")
        within(ref, "one workgroup")
        for keep in keeps:
            s, idx, nxt, _ = run_query(q, H, P, keep, nat.QUERY_MEAN)
            assert torch.equal(bits(s), bits(ref)), what
            check_selection(s, idx, nxt, keep, P, f"{what} keep={keep}")
            _, idx2, nxt2, _ = run_query(q, H, P, keep, nat.QUERY_MEAN, want_scores=False)
            assert torch.equal(idx2, idx) and torch.equal(bits(nxt2), bits(nxt)), what
        lib().rajni_debug_force_score_two_pass(1)
        for keep in (0,) + tuple(keeps):
            s, idx, nxt, _ = run_query(q, H, P, keep, nat.QUERY_MEAN)
            assert torch.equal(bits(s), bits(ref)), f"{what}: the two-pass layout gives other bits"
            if keep:
                check_selection(s, idx, nxt, keep, P, f"{what} keep={keep}, two-pass")
        lib().rajni_debug_force_score_two_pass(0)
        # ---- the tiled path (a launch for the mean query, the tiles, the finish): within the budget, the same bits twice
        lib().rajni_debug_force_score_tiled(1)
        t1, _, _, nbytes = run_query(q, H, P, 0, nat.QUERY_MEAN)
        assert nbytes >= B * H * D * 4
        within(t1, "tiled")
        for keep in keeps:
            s, idx, nxt, _ = run_query(q, H, P, keep, nat.QUERY_MEAN)
            assert torch.equal(bits(s), bits(t1)), f"{what}: the tiled path is not repeatable"
            check_selection(s, idx, nxt, keep, P, f"{what} keep={keep}, tiled")
    finally:
        lib().rajni_debug_force_score_two_pass(0)
        lib().rajni_debug_force_score_tiled(0)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("B,N,H,D,P,keeps", SHAPES, ids=IDS)
def test_batch_position_does_not_change_the_bits(B, N, H, D, P, keeps, dt):
    qkv = dev(nq.query_qkv("qcancel", B, N, H, D, dt), dt)
    try:
        for tiled in (0, 1):
            lib().rajni_debug_force_score_tiled(tiled)
            full, idx, _, _ = run_query(qkv, H, P, keeps[0], nat.QUERY_MEAN)
            one, idx1, _, _ = run_query(qkv[B - 1:].contiguous(), H, P, keeps[0], nat.QUERY_MEAN)
            assert torch.equal(bits(one), bits(full[B - 1:])) and torch.equal(idx1, idx[B - 1:]), (tiled, N, dt)
    finally:
        lib().rajni_debug_force_score_tiled(0)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("B,N,H,D,P,keeps", SHAPES, ids=IDS)
def test_the_class_query_through_the_new_entry_point_is_the_old_one(B, N, H, D, P, keeps, dt):
    """RAJNI_QUERY_CLS gives the bits of rajni_score_select_ws (P >= 1); with P = 0, which that entry point refuses, the scores
    are still its scores and every token is ranked"""
    qkv = dev(nm.importance_qkv("peaked", B, N, H, D, dt), dt)
    code = nat.dtype_code(qkv.dtype)
    keep = min(keeps[0], N - max(P, 1))
    try:
        for tiled in (0, 1):
            lib().rajni_debug_force_score_tiled(tiled)
            nbytes = lib().rajni_score_select_workspace_bytes(B, N, H, D, code)
            assert lib().rajni_score_select_query_workspace_bytes(B, N, H, D, code, nat.QUERY_CLS) == nbytes
            ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes else None
            Pw = max(P, 1)
            s0, i0, n0 = (torch.empty((B, N), dtype=qkv.dtype, device=DEV), torch.empty((B, Pw + keep), dtype=torch.int32, device=DEV),
                          torch.empty((B, Pw + keep), dtype=qkv.dtype, device=DEV))
            nat.check(lib().rajni_score_select_ws(qkv.data_ptr(), B, N, H, D, 1e-6, Pw, keep, s0.data_ptr(), i0.data_ptr(), n0.data_ptr(),
                                                  code, nat.ptr(ws), nbytes, stream()), "rajni_score_select_ws")
            s1, i1, n1, _ = run_query(qkv, H, Pw, keep, nat.QUERY_CLS)
            assert torch.equal(bits(s1), bits(s0)) and torch.equal(i1, i0) and torch.equal(bits(n1), bits(n0)), (tiled, N, dt)
            if P == 0:
                s2, i2, n2, _ = run_query(qkv, H, 0, keep, nat.QUERY_CLS)
                assert torch.equal(bits(s2), bits(s0))
                check_selection(s2, i2, n2, keep, 0, f"class query, P = 0, N={N} {dt}")
    finally:
        lib().rajni_debug_force_score_tiled(0)


def test_the_fixture_recorded_from_the_reference():
    """identical query rows: the mean query is the reference's class query.  The bars of
    tests/test_gpu_kernels.py::test_importance_golden_cases for its fixture: 6e-3 of the largest score, against the restatement and
    against the reference's recorded scores (fp32 here: the fixture's query rows are not bf16 values)"""
    for c, qkv, ref in nq.load_fixture():
        q = dev(qkv, "fp32")
        want = nq.importance_scores(qkv, c["H"])
        try:
            for tiled in (0, 1):
                lib().rajni_debug_force_score_tiled(tiled)
                got = host(run_query(q, c["H"], 0, 0, nat.QUERY_MEAN)[0])
                cls = host(run_query(q, c["H"], 0, 0, nat.QUERY_CLS)[0])
                for other, name in ((want, "restatement"), (ref.astype(np.float64), "reference fixture"), (cls, "the class query")):
                    scale, err = np.abs(other).max(), np.abs(got - other).max()
                    print(f"[noclass] fixture N={c['N']} H={c['H']} D={c['D']} tiled={tiled} vs {name}: {err / scale:.3g}")
                    assert err <= 6e-3 * scale, (c, tiled, name)
                # the sums of identical rows are exact in any order: the mean query IS the class query, to the bit
                assert np.array_equal(got, cls), (c, tiled)
        finally:
            lib().rajni_debug_force_score_tiled(0)


def test_python_surface():
    qkv = nm.importance_qkv("vflat", 2, 33, 2, 64, "bf16")
    q = dev(qkv, "bf16")
    ref, _, _, _ = run_query(q, 2, 0, 0, nat.QUERY_MEAN)
    assert torch.equal(ops.importance(q, 2, query="mean"), ref) and torch.equal(compute_importance_query(q, 2, query="mean"), ref)
    assert torch.equal(compute_importance_query(q, 2), ops.importance(q, 2))
    for P, query in ((0, "mean"), (4, "mean"), (0, "cls")):
        s, idx, nxt = ops.score_select(q, 2, 9, num_prefix=P, query=query)
        assert torch.equal(s, ref if query == "mean" else ops.importance(q, 2)) and tuple(idx.shape) == (2, P + 9)
        check_selection(s, idx, nxt, 9, P, f"ops.score_select P={P} {query}")
        i2, n2 = ops.select_topk(s, 9, num_prefix=P)
        assert torch.equal(i2, idx) and torch.equal(n2, nxt)
    with pytest.raises(ValueError, match="query must be"):
        ops.score_select(q, 2, 9, query="max")


@pytest.mark.parametrize("tiled", [0, 1], ids=["one_workgroup", "tiled"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_poisoned_buffers_with_no_prefix_token(dt, tiled):
    """qkv, the outputs and the scratch inside poisoned arenas (tests/guarded.py): keep_idx [B, keep], next_scores [B, keep] and
    scores_out [B, N] written in full and nowhere else with P = 0, the scratch's guards intact, the input untouched"""
    B, N, H, D = 3, 37, 2, 64
    td = nm.TORCH[dt]
    qkv = dev(nm.importance_qkv("voutlier", B, N, H, D, dt), dt)
    qg = Guarded((B, N, 3 * H * D), td, DEV).fill_(qkv)
    before = qg.arena.clone()
    code = nat.dtype_code(td)
    lib().rajni_debug_force_score_tiled(tiled)
    try:
        nbytes = lib().rajni_score_select_query_workspace_bytes(B, N, H, D, code, nat.QUERY_MEAN)
        assert (nbytes > 0) == bool(tiled)
        wg = Guarded((max(nbytes, 256),), torch.uint8, DEV)
        ref = None
        for keep in (1, 18, N):
            what = f"score_select_query P=0 N={N} keep={keep} {dt} tiled={tiled}"
            sg, ig, ng = Guarded((B, N), td, DEV), Guarded((B, keep), torch.int32, DEV), Guarded((B, keep), td, DEV)
            nat.check(lib().rajni_score_select_query(qg.ptr(), B, N, H, D, 1e-6, 0, keep, nat.QUERY_MEAN, sg.ptr(), ig.ptr(), ng.ptr(),
                                                     code, wg.ptr() if nbytes else None, nbytes, stream()), "rajni_score_select_query")
            torch.cuda.synchronize()
            for gd, name in ((sg, "scores_out"), (ig, "keep_idx"), (ng, "next_scores")):
                gd.check(f"{what}: {name}")
            wg.check(f"{what}: workspace", written=False)
            ref = sg.t.clone() if ref is None else ref
            assert torch.equal(bits(sg.t), bits(ref)), what
            check_selection(sg.t, ig.t, ng.t, keep, 0, what)
        assert torch.equal(qg.arena, before), "the qkv arena changed"
        want, bud, _ = nq.importance_budget(host(qkv), H, dt)
        nm.assert_within(host(ref), want, bud, f"poisoned arenas {dt} tiled={tiled}")
    finally:
        lib().rajni_debug_force_score_tiled(0)
