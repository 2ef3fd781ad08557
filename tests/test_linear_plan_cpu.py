"""rajni_linear's host side without a GPU, through the dry-run hook rajni_debug_linear_plan (include/rajni_hip_debug.h): the
hook runs the argument checks, the format / epilogue resolution and the tiling choice of rajni_linear for a given CU count and
returns before the launch.  Two halves:

  * every refusal of rajni_linear - return code, message text, and which one wins where two apply;
  * the tiling choice (tiling, tile counts, N block, grid, dynamic LDS) against a Python restatement of the decision rule
    of csrc/gemm.hip as it stood before the choice was separated from the launch, plus literal anchors that the comments
    next to that rule record, so that the restatement cannot drift together with the code.

The pointers handed in are fake (non-null, 16-byte aligned): the hook checks them and never follows them.  rajni_linear
itself is never called here."""
import ctypes as C
import itertools

import pytest

from rajni_amd import _native as nat

F32, BF16, F16 = nat.RAJNI_F32, nat.RAJNI_BF16, nat.RAJNI_F16
BIAS, GELU, RESID = nat.EPI_BIAS, nat.EPI_BIAS_GELU, nat.EPI_BIAS_RESID
OK, INVALID, UNSUPPORTED = 0, 1, 2
SMALL, T_F32, WIDE, MID, F8_STREAM, F8_WIDE = (nat.TILING_SMALL, nat.TILING_F32, nat.TILING_WIDE, nat.TILING_MID,
                                               nat.TILING_F8_STREAM, nat.TILING_F8_WIDE)
PTR = 0x10000           # fake addresses, 16-byte aligned, never followed
NBLK_DEFAULT = 1600 * 1024


def args(M=2048, N=768, K=768, epilogue=BIAS, dtype=BF16, stream_f32=0, resid=False, w_scale=False, x_scale=False,
         y_scale=False, r_idx=False, **over):
    a = nat.LinearArgs()
    a.x, a.w, a.y, a.bias = PTR, 2 * PTR, 3 * PTR, 4 * PTR
    a.lda, a.ldw, a.ldc, a.ldr = K, K, N, N
    a.M, a.N, a.K, a.epilogue, a.dtype, a.stream_f32 = M, N, K, epilogue, dtype, stream_f32
    a.resid = (5 * PTR if resid is True else resid) if resid else None
    a.w_scale = 6 * PTR if w_scale else None
    a.x_scale = 7 * PTR if x_scale else None
    a.y_scale = 8 * PTR if y_scale else None
    a.r_idx = 9 * PTR if r_idx else None
    for k, v in over.items():
        setattr(a, k, v)
    return a


def plan(a, cus=256):
    out = nat.LinearPlan()
    rc = nat.lib().rajni_debug_linear_plan(C.byref(a), cus, C.byref(out))
    return rc, out, nat.lib().rajni_last_error().decode()


@pytest.fixture
def hooks():
    """sets the tiling / N-block hooks for a case and restores the defaults"""
    lib = nat.lib()

    def set_hooks(force=0, force_f8=0, nblk=NBLK_DEFAULT):
        lib.rajni_debug_force_gemm_tiling(force)
        lib.rajni_debug_force_f8_tiling(force_f8)
        lib.rajni_debug_set_gemm_nblock_bytes(nblk)
        lib.rajni_debug_set_persistent_workgroups(0)
    yield set_hooks
    set_hooks()


# ---------------------------------------------------------------------------------------------------------------
# refusals: (case, code, message substring).  Listed in the order rajni_linear checks; where a case breaks two rules the
# expected message is the earlier one's.
# ---------------------------------------------------------------------------------------------------------------
F8 = dict(w_scale=True, x_scale=True, K=1024)      # a valid fp8 x fp8 call
W8 = dict(w_scale=True)                            # a valid fp8-weight call
RESID_MSG = "rajni_linear: RESID epilogue needs resid and ldr % 8 == 0"
RESID_MSG_F8 = "rajni_linear: RESID epilogue needs resid, ldr % 8 == 0 and no y_scale"
REFUSALS = [
    ("bad dtype", args(dtype=7), INVALID, "rajni_linear: bad dtype 7"),
    ("bad dtype before null pointer", args(dtype=7, x=None), INVALID, "rajni_linear: bad dtype 7"),
    ("fp16 + w_scale", args(dtype=F16, w_scale=True), UNSUPPORTED, "need a bf16 model (dtype fp16 given)"),
    ("fp16 + x_scale", args(dtype=F16, x_scale=True), UNSUPPORTED, "need a bf16 model (dtype fp16 given)"),
    ("fp16 + scales before null pointer", args(dtype=F16, w_scale=True, y=None), UNSUPPORTED, "need a bf16 model (dtype fp16 given)"),
    ("null x", args(x=None), INVALID, "rajni_linear: null pointer"),
    ("null w", args(w=None), INVALID, "rajni_linear: null pointer"),
    ("null y", args(y=None), INVALID, "rajni_linear: null pointer"),
    ("null pointer before shape", args(y=None, K=100), INVALID, "rajni_linear: null pointer"),
    ("K % 64", args(K=100, lda=104, ldw=104), INVALID, "M,N>0 and K % 64 == 0 required (M=2048 N=768 K=100)"),
    ("M = 0", args(M=0), INVALID, "M,N>0 and K % 64 == 0 required (M=0 N=768 K=768)"),
    ("N < 0", args(N=-1, ldc=8), INVALID, "M,N>0 and K % 64 == 0 required"),
    ("lda % 8", args(lda=772), INVALID, "leading dimensions must be multiples of 8 elements"),
    ("ldw % 8", args(ldw=772), INVALID, "leading dimensions must be multiples of 8 elements"),
    ("ldc % 8", args(ldc=772), INVALID, "leading dimensions must be multiples of 8 elements"),
    ("shape before leading dimensions", args(K=100, lda=101), INVALID, "K % 64 == 0 required"),
    ("x alignment", args(x=PTR + 8), INVALID, "pointers must be 16-byte aligned"),
    ("resid alignment", args(epilogue=RESID, resid=5 * PTR + 4), INVALID, "pointers must be 16-byte aligned"),
    ("leading dimensions before alignment", args(lda=772, w=2 * PTR + 2), INVALID, "leading dimensions"),
    # fp8 x fp8
    ("x_scale without w_scale", args(x_scale=True, K=1024), INVALID, "fp8 activations (x_scale) need fp8 weights (w_scale) and dtype bf16"),
    ("x_scale with fp32", args(dtype=F32, **F8), INVALID, "fp8 activations (x_scale) need fp8 weights (w_scale) and dtype bf16"),
    ("fp8 x fp8 K % 256", args(w_scale=True, x_scale=True, K=320), UNSUPPORTED, "needs K % 256 == 0 and K >= 512 (K=320)"),
    ("fp8 x fp8 K < 512", args(w_scale=True, x_scale=True, K=256), UNSUPPORTED, "needs K % 256 == 0 and K >= 512 (K=256)"),
    ("w_scale before fp8 x fp8 K", args(x_scale=True, K=320), INVALID, "need fp8 weights (w_scale)"),
    ("fp8 x fp8 K before lda", args(w_scale=True, x_scale=True, K=320, lda=328), UNSUPPORTED, "needs K % 256 == 0"),
    ("fp8 x fp8 lda % 16", args(lda=1032, **F8), INVALID, "fp8 operands need lda, ldw % 16 == 0 (bytes)"),
    ("fp8 x fp8 ldw % 16", args(ldw=1032, **F8), INVALID, "fp8 operands need lda, ldw % 16 == 0 (bytes)"),
    ("fp8 x fp8 BIAS + y_scale", args(y_scale=True, **F8), UNSUPPORTED, "an fp8 output (y_scale) exists for the GELU epilogue only"),
    ("fp8 x fp8 GELU without y_scale", args(epilogue=GELU, **F8), UNSUPPORTED, "GELU epilogue writes e4m3 (y_scale required, ldc % 16 == 0 bytes)"),
    ("fp8 x fp8 GELU ldc % 16", args(epilogue=GELU, y_scale=True, ldc=776, **F8), UNSUPPORTED, "GELU epilogue writes e4m3 (y_scale required"),
    ("fp8 x fp8 RESID without resid", args(epilogue=RESID, **F8), INVALID, RESID_MSG_F8),
    ("fp8 x fp8 RESID ldr % 8", args(epilogue=RESID, resid=True, ldr=772, **F8), INVALID, RESID_MSG_F8),
    ("fp8 x fp8 RESID + y_scale", args(epilogue=RESID, resid=True, y_scale=True, **F8), INVALID, RESID_MSG_F8),
    ("fp8 x fp8 unknown epilogue", args(epilogue=3, **F8), INVALID, "rajni_linear: unknown epilogue 3"),
    ("fp8 x fp8 lda before epilogue", args(epilogue=3, lda=1032, **F8), INVALID, "fp8 operands need lda"),
    # y_scale belongs to fp8 x fp8
    ("y_scale without x_scale", args(y_scale=True), INVALID, "rajni_linear: y_scale without x_scale"),
    ("y_scale without x_scale before the fp8-weight checks", args(y_scale=True, w_scale=True, ldw=776), INVALID, "y_scale without x_scale"),
    ("y_scale without x_scale before the epilogue", args(y_scale=True, epilogue=RESID), INVALID, "y_scale without x_scale"),
    # fp8 weights on bf16
    ("fp8 weights with fp32", args(dtype=F32, **W8), UNSUPPORTED, "rajni_linear: fp8 weights need bf16 activations"),
    ("fp8 weights ldw % 16", args(ldw=776, **W8), INVALID, "rajni_linear: fp8 weights need ldw % 16 == 0"),
    ("fp8 weights: dtype before ldw", args(dtype=F32, ldw=776, **W8), UNSUPPORTED, "fp8 weights need bf16 activations"),
    ("fp8 weights RESID without resid", args(epilogue=RESID, **W8), INVALID, RESID_MSG),
    ("fp8 weights RESID ldr % 8", args(epilogue=RESID, resid=True, ldr=772, **W8), INVALID, RESID_MSG),
    ("fp8 weights unknown epilogue", args(epilogue=-1, **W8), INVALID, "rajni_linear: unknown epilogue -1"),
    ("fp8 weights: ldw before epilogue", args(epilogue=3, ldw=776, **W8), INVALID, "fp8 weights need ldw"),
    # fp32
    ("fp32 RESID without resid", args(dtype=F32, epilogue=RESID), INVALID, "rajni_linear: RESID epilogue needs resid"),
    ("fp32 unknown epilogue", args(dtype=F32, epilogue=3), INVALID, "rajni_linear: unknown epilogue 3"),
    # bf16 / fp16
    ("bf16 RESID without resid", args(epilogue=RESID), INVALID, RESID_MSG),
    ("bf16 RESID ldr % 8", args(epilogue=RESID, resid=True, ldr=772), INVALID, RESID_MSG),
    ("fp16 RESID without resid", args(dtype=F16, epilogue=RESID, stream_f32=1), INVALID, RESID_MSG),
    ("fp16 RESID ldr % 8", args(dtype=F16, epilogue=RESID, resid=True, ldr=772), INVALID, RESID_MSG),
    ("bf16 unknown epilogue", args(epilogue=3), INVALID, "rajni_linear: unknown epilogue 3"),
    ("fp16 unknown epilogue", args(dtype=F16, epilogue=4), INVALID, "rajni_linear: unknown epilogue 4"),
]


@pytest.mark.parametrize("name,a,code,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_keep_code_message_and_precedence(name, a, code, msg):
    rc, _, err = plan(a)
    assert rc == code and msg in err, (name, rc, err)


def test_fp32_resid_message_is_the_short_one():
    """the fp32 RESID refusal names resid only, and - unlike every other format - fp32 accepts ldr % 8 != 0"""
    rc, _, err = plan(args(dtype=F32, epilogue=RESID))
    assert rc == INVALID and err == "rajni_linear: RESID epilogue needs resid"
    rc, out, _ = plan(args(dtype=F32, epilogue=RESID, resid=True, ldr=772))
    assert rc == OK and out.tiling == T_F32


def test_hook_refuses_its_own_bad_arguments():
    out = nat.LinearPlan()
    assert nat.lib().rajni_debug_linear_plan(None, 256, C.byref(out)) == INVALID
    assert nat.lib().rajni_last_error().decode() == "rajni_linear: null args"
    assert nat.lib().rajni_debug_linear_plan(C.byref(args()), 0, C.byref(out)) == INVALID
    assert nat.lib().rajni_debug_linear_plan(C.byref(args()), 256, None) == INVALID


def test_accepted_calls_of_every_format():
    for a, tiling in [(args(), MID), (args(dtype=F16), MID), (args(**W8), MID), (args(dtype=F32), T_F32), (args(**F8), F8_STREAM),
                      (args(epilogue=GELU, y_scale=True, **F8), F8_STREAM), (args(epilogue=RESID, resid=True, **F8), F8_STREAM),
                      (args(epilogue=RESID, resid=True, stream_f32=1, **W8), MID), (args(M=1), SMALL)]:
        rc, out, err = plan(a)
        assert rc == OK and out.tiling == tiling, (rc, err, out.tiling)


# ---------------------------------------------------------------------------------------------------------------
# the decision rule, restated from csrc/gemm.hip (launch_gemm, launch_gemm_f8, f32::launch and their helpers) as of the
# commit before the split.  C integer division of non-negative values = //; doubles = Python floats.
# ---------------------------------------------------------------------------------------------------------------
KIB = 1024


def ceil_div(a, b):
    return (a + b - 1) // b


def n_block(tiles_n, tiles_m, bn, K, wbytes, cus, nblk_bytes):
    if nblk_bytes < 0:
        return min(-nblk_bytes, tiles_n)
    if nblk_bytes == 0:
        return tiles_n
    fit = nblk_bytes // (bn * K * wbytes)
    if fit < 1 or fit >= tiles_n:
        return tiles_n
    blocks = ceil_div(tiles_n, fit)
    if tiles_n * tiles_m // cus < 2 * blocks:
        return tiles_n
    return ceil_div(tiles_n, blocks)


def eff_rounds(tiles, cus):
    full = tiles // cus
    frac = float(tiles) / float(cus) - float(full)
    return float(full) + (0.6 + 0.4 * frac if frac > 0.0 else 0.0)


def wide_wins_on_rounds(M, N, cus):
    rows = ceil_div(M, 256)
    return 1.83 * eff_rounds(rows * ceil_div(N, 256), cus) < eff_rounds(rows * ceil_div(N, 128), cus)


def stream_grid(total, cus):
    return min(total, cus)


def expect_16bit(M, N, K, epi, sf32, w8, cus, force, nblk_bytes, resid_elems):
    """launch_gemm<EPI, ALOAD_PLAIN, SF32, W8>: (tiling, tiles_n, total_tiles, nblk, grid, lds)"""
    nat_resid = bool(sf32) and epi == RESID
    mode = force
    if mode in (4, 5) and M < 256:
        mode = 1
    if mode == 4 and K < 192:
        mode = 1
    if mode == 5 and K < 256:
        mode = 1
    mid_ok = not nat_resid or resid_elems < (1 << 31)
    if mode == 5 and not mid_ok:
        mode = 1
    if mode == 0:
        if M >= 1024 and N >= 1536 and K >= 192:
            mode = 4
        elif M >= 1024 and K >= 256:
            mode = 4 if (K > N and K >= 1536 and wide_wins_on_rounds(M, N, cus)) else (5 if mid_ok else 1)
        else:
            mode = 1
    tstore = epi in (BIAS, GELU)                      # RAJNI_TSTORE = 1
    tiles_m = ceil_div(M, 256)
    if mode == 4:
        stages = 2 * (32 * KIB + 256 * 64 * (1 if w8 else 2))          # wide::Cfg<4, 2, W8>::LDS_BYTES
        lds = stages + (8 * 2048 if (tstore or (nat_resid and not w8)) else 0)
        tiles_n = ceil_div(N, 256)
        total = tiles_n * tiles_m
        return WIDE, tiles_n, total, n_block(tiles_n, tiles_m, 256, K, 2, cus, nblk_bytes), stream_grid(total, cus), lds
    if mode == 5:
        stages = 3 * (32 * KIB + 128 * 64 * (1 if w8 else 2))          # wide::Cfg<2, 3, W8>::LDS_BYTES
        lds = stages + (8 * 2048 if (nat_resid or tstore) else 0)
        tiles_n = ceil_div(N, 128)
        total = tiles_n * tiles_m
        return MID, tiles_n, total, n_block(tiles_n, tiles_m, 128, K, 2, cus, nblk_bytes), stream_grid(total, cus), lds
    tiles_n = ceil_div(N, 128)
    total = tiles_n * ceil_div(M, 128)
    return SMALL, tiles_n, total, 0, total, 64 * KIB                   # small::LDS_BYTES; nblk stays 0


def expect_f8(M, N, K, epi, sf32, cus, force_f8, nblk_bytes):
    """launch_gemm_f8<EPI, SF32>; epi GELU is the e4m3-output epilogue"""
    nat_resid = bool(sf32) and epi == RESID
    tiles_m = ceil_div(M, 256)
    if epi in (BIAS, GELU):
        def rounds_ok():
            rounds = float(tiles_m) * ceil_div(N, 256) / cus
            frac = rounds - int(rounds)
            return not (rounds < 8.0 and 0.0 < frac < 0.2)
        want = force_f8 == 2 or (force_f8 == 0 and M >= 1024 and N >= 1536 and (epi == GELU or rounds_ok()))   # RAJNI_F8W_LINES = 1
        if K >= 384 and want:
            tiles_n = ceil_div(N, 256)
            total = tiles_n * tiles_m
            lds = 2 * (32 * KIB + 32 * KIB) + (8 * 4096 if epi == BIAS else 0)
            return F8_WIDE, tiles_n, total, n_block(tiles_n, tiles_m, 256, K, 1, cus, nblk_bytes), stream_grid(total, cus), lds
    tiles_n = ceil_div(N, 128)
    total = tiles_n * tiles_m
    lds = 3 * (32 * KIB + 16 * KIB) + (8 * 2048 if (nat_resid or epi == BIAS) else 0)
    return F8_STREAM, tiles_n, total, n_block(tiles_n, tiles_m, 128, K, 1, cus, nblk_bytes), stream_grid(total, cus), lds


def expect_f32(M, N):
    tiles_n = ceil_div(N, 128)
    total = tiles_n * ceil_div(M, 128)
    return T_F32, tiles_n, total, 0, total, 2 * 2 * 128 * 32 * 4       # f32::LDS_BYTES


def got(a, cus):
    rc, o, err = plan(a, cus)
    assert rc == OK, err
    return o.tiling, o.tiles_n, o.total_tiles, o.nblk, o.grid, o.lds_bytes


MS = [1, 255, 256, 1023, 1024, 256 * 87, 256 * 121, 256 * 152, 256 * 173, 256 * 197, 512 * 197, 64 * 577]
NK = sorted({nk for c, h in [(768, 3072), (1024, 4096), (1280, 5120)]          # ViT-B, ViT-L, ViT-H
             for nk in [(3 * c, c), (c, c), (h, c), (c, h), (1000, c)]})         # QKV, proj, FC1, FC2, head
CUS = [256, 64]
NBLKS = [NBLK_DEFAULT, 0, -2]
EPIS = [(BIAS, 0), (GELU, 0), (RESID, 0), (RESID, 1)]


@pytest.mark.parametrize("fmt", ["bf16", "fp16", "w8"])
@pytest.mark.parametrize("force", [0, 1, 4, 5])
def test_choice_16bit_matches_the_rule(hooks, fmt, force):
    extra = dict(dtype=F16) if fmt == "fp16" else dict(w_scale=True) if fmt == "w8" else {}
    for nblk in NBLKS:
        hooks(force=force, nblk=nblk)
        for (N, K), M, cus, (epi, sf32) in itertools.product(NK, MS, CUS, EPIS):
            a = args(M, N, K, epi, stream_f32=sf32, resid=epi == RESID, **extra)
            want = expect_16bit(M, N, K, epi, sf32, fmt == "w8", cus, force, nblk, M * N)
            assert got(a, cus) == want, (fmt, force, nblk, M, N, K, epi, sf32, cus)


@pytest.mark.parametrize("force_f8", [0, 1, 2])
def test_choice_fp8_matches_the_rule(hooks, force_f8):
    for nblk in NBLKS:
        hooks(force_f8=force_f8, force=4, nblk=nblk)      # the bf16 hook must not reach the fp8 x fp8 kernels
        for (N, K), M, cus, (epi, sf32) in itertools.product(NK, MS, CUS, EPIS):
            a = args(M, N, K, epi, stream_f32=sf32, resid=epi == RESID, y_scale=epi == GELU, w_scale=True, x_scale=True,
                     ldc=(N + 15) // 16 * 16)        # the e4m3 output wants ldc % 16 (the head: N = 1000)
            assert got(a, cus) == expect_f8(M, N, K, epi, sf32, cus, force_f8, nblk), (force_f8, nblk, M, N, K, epi, sf32, cus)


def test_choice_fp32_is_one_workgroup_per_tile(hooks):
    for force in (0, 4, 5):
        hooks(force=force)
        for (N, K), M, epi in itertools.product(NK, MS, (BIAS, GELU, RESID)):
            a = args(M, N, K, epi, dtype=F32, resid=epi == RESID)
            assert got(a, 256) == expect_f32(M, N), (force, M, N, K, epi)


@pytest.mark.parametrize("force", [0, 5, 4])
@pytest.mark.parametrize("fmt", ["bf16", "w8"])
def test_residual_tensor_of_2_31_elements_leaves_the_256x128_tiling(hooks, fmt, force):
    """mid_ok: the 256 x 128 tiling's fp32-stream RESID epilogue keeps 32-bit element offsets into the residual tensor -
    resid_rows * ldr >= 2^31 goes to 128 x 128 (by shape and under the forced hook); resid_rows = M, or (M / r_np) * r_nsrc
    with gathered rows.  The bf16 stream and the 256 x 256 tiling are not affected."""
    hooks(force=force)
    extra = dict(w_scale=True) if fmt == "w8" else {}
    N = K = 768
    direct = [(2796202, {}), (2796203, {})]                                          # M * 768 = 2^31 - 512, 2^31 + 256
    gathered = [(256 * 152, dict(r_idx=True, r_np=152, r_nsrc=n)) for n in (10922, 10923)]    # 256 * r_nsrc * 768 around 2^31
    for M, gather in direct + gathered:
        elems = (M // gather["r_np"]) * gather["r_nsrc"] * N if gather else M * N
        assert (elems < 1 << 31) == (M == 2796202 or gather.get("r_nsrc") == 10922)
        for sf32 in (1, 0):
            a = args(M, N, K, RESID, stream_f32=sf32, resid=True, **extra, **gather)
            want = expect_16bit(M, N, K, RESID, sf32, fmt == "w8", 256, force, NBLK_DEFAULT, elems)
            assert got(a, 256) == want
            small = bool(sf32) and elems >= 1 << 31 and force != 4
            assert want[0] == (SMALL if small else WIDE if force == 4 else MID)


def test_anchors_recorded_next_to_the_rule(hooks):
    """picks that the comments in csrc/gemm.hip record (measured on the chip), as literals"""
    hooks()
    B256 = 256 * 197                                                                         # ViT-B, batch 256
    assert got(args(B256, 2304, 768), 256)[0] == WIDE                                        # QKV
    assert got(args(B256, 3072, 768, GELU), 256)[0] == WIDE                                  # FC1
    assert got(args(B256, 768, 768, RESID, resid=True, stream_f32=1), 256)[0] == MID         # proj
    assert got(args(B256, 768, 3072, RESID, resid=True, stream_f32=1), 256)[0] == MID        # fc2: 591 wide tiles = 2.3 rounds
    assert got(args(256 * 152, 768, 3072, RESID, resid=True, stream_f32=1), 256)[0] == WIDE  # fc2 at 152 tokens (wide_wins_on_rounds)
    assert got(args(512 * 197, 768, 3072, RESID, resid=True, stream_f32=1), 256)[0] == WIDE  # fc2 at batch 512
    assert got(args(256, 1000, 768), 256)[0] == SMALL                                        # head
    f8 = dict(w_scale=True, x_scale=True)
    assert got(args(B256, 2304, 768, **f8), 256)[0] == F8_WIDE                               # fp8 QKV: whole-line epilogue
    assert got(args(256 * 173, 2304, 768, **f8), 256)[0] == F8_STREAM                        # 173 * 9 / 256 = 6.08 rounds
    assert got(args(512 * 87, 2304, 768, **f8), 256)[0] == F8_STREAM                         # 174 * 9 / 256 = 6.12 rounds
    assert got(args(B256, 3072, 768, GELU, y_scale=True, **f8), 256)[0] == F8_WIDE           # fp8 FC1
    assert got(args(256 * 173, 3072, 768, GELU, y_scale=True, **f8), 256)[0] == F8_WIDE      # ... whatever the rounds
    assert got(args(B256, 768, 3072, RESID, resid=True, stream_f32=1, **f8), 256)[0] == F8_STREAM
    # dynamic LDS of the instantiations that fill the workgroup's 160 KiB: stages + 8 waves of scratch
    assert got(args(B256, 768, 768, RESID, resid=True, stream_f32=1), 256)[5] == 144 * KIB + 16 * KIB
    assert got(args(B256, 2304, 768, **f8), 256)[5] == 128 * KIB + 32 * KIB
    assert got(args(B256, 2304, 768), 256)[5] == 128 * KIB + 16 * KIB
    assert got(args(256 * 152, 768, 3072, RESID, resid=True), 256)[5] == 128 * KIB           # bf16 stream: no transpose
