"""-m gpu: the write promises of include/brepgen_hip.h, checked for every exported kernel entry point.

Every test calls an entry point with its inputs in strided, sentinel-padded buffers and its outputs in guard-banded, sentinel-filled
ones (tests/guarded.py), then asserts three things: every logical output element was written, nothing outside the logical region
(front guard, rear guard, the padding of every row) was touched, and the logical result is the operation's value -- an fp64 reference
on the already-rounded operands (tests/parity_cases.py) under the tolerance the suite already asserts for that operation and dtype
(tests/test_gpu_parity.py, tests/test_gpu_round*.py), or the bit-exact restatement where the existing test uses one.

Section A also asserts the kernel that served the call (bg_profile_begin / bg_profile_end report it), so that a dispatch change cannot
silently move a case onto another kernel.  The profiler books the narrow 128 x 64 and the small-launch 64 x 64 instantiations of the
generic kernel under one name, and the generic and the persistent 128 x 128 kernels under another; the knobs P256_MODE, SPLIT_PIPE, SMALL_TILES and
the strides select between those, as launch16 (csrc/gemm_16bit.hip) documents.  A strided call whose strides change only addresses
(every stride a multiple of 8, same keys) must equal the dense call on the same operands bit for bit; where the strides change the
dispatch (ldc = 770 / 772: scalar or 8-byte stores) only the fp64 tolerance is required and the bit comparison is printed.
"""
import math

import pytest
import torch

from gpu_check import tune  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
K_GENERIC = "gemm16_kernel(generic: 128x64 / 64x64 tiles)"
K_128 = "gemm16_persistent_kernel(128x128)"
K_SPLIT_PIPE = "gemm16_split_pipe_kernel(128x128)"
K_P256 = "gemm16_p256_kernel(256x256)"
K_P256_SPLIT = "gemm16_p256_kernel(256x256, split-residual launches)"
K_F32 = "gemm_f32"


@pytest.fixture(scope="module")
def pc():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import parity_cases
    return parity_cases


def _out_tol(e, out_dtype):
    """The suite's bound for one GEMM result: 2e-5 (exact products, fp32 accumulation, K <= 1024) for an fp32 output; one rounding of
    the output for a 16-bit one -- bf16 4e-3 |y|max + 1e-6 (test_gemm_bf16_epilogues), fp16 its 11 significand bits: 2^-11 = 4.9e-4."""
    if out_dtype == F32:
        return 2e-5
    return (4e-3 if out_dtype == BF16 else 4.9e-4) * e["ref_absmax"] + 1e-6


def _check_plain(e, out_dtype, kernel, what, must_equal_dense, inplace=False):
    print(f"{what}: max_abs {e['max_abs']:.3g} kernels {e['kernels']} bits equal to the dense call: {e['bits_equal']}")
    if not inplace:
        e["out"].assert_fully_written(what)
    e["out"].assert_untouched(what)
    assert e["kernels"] == [kernel], (what, e["kernels"])
    assert e["finite"] and e["max_abs"] < _out_tol(e, out_dtype), (what, e["max_abs"])
    if must_equal_dense:
        assert e["bits_equal"], what


# ==== A. 16-bit GEMM ===============================================================================================================
@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M", [1, 127, 129])
def test_narrow_gemm_writes_only_the_valid_columns(pc, dt, M):
    """N_pad = 64 (fc_out.3: 6 / 18 / 48 real columns), the 128 x 64 instantiation with the scalar epilogue: `only columns < N are
    written` for every row stride -- tight, odd, the padded width itself and beyond it."""
    for N in (1, 6, 18, 48, 63):
        for ldc in (N, N + 1, 64, 72):
            for odt in (F32, dt):
                for add_mode, ld_add in ((None, None), ("resid", N), (30, N + 3), ("resid", N + 3), (30, N), ("alias", None)):
                    if add_mode == "alias" and odt != F32:
                        continue                                   # (the addend is fp32: it can only alias an fp32 output)
                    e = pc.gemm_abi_case(M, 64, 768, dt, n_valid=N, ldc=ldc, out_dtype=odt, add_mode=add_mode, ld_add=ld_add, seed=N)
                    # (N < N_pad: the scalar epilogue for every stride -- the strides change addresses only)
                    _check_plain(e, odt, K_GENERIC, f"narrow M={M} N={N} ldc={ldc} out={odt} add={add_mode}/{ld_add}", True,
                                 inplace=add_mode == "alias")


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M", [1, 63, 65, 300])
def test_small_launch_gemm_with_strides(pc, dt, M):
    """< 160 tiles of 128 x 128: the 64 x 64 instantiation (the library's own choice).  (776, 776) moves addresses only; ldc = 772
    keeps the vector epilogue for rows that are 8- but not 16-byte multiples apart (16-bit output); ldc = 770 and ld_add = 770 take the
    scalar epilogue with N == N_pad."""
    for lda, ldc in ((768, 768), (776, 776), (768, 772), (768, 770)):
        same = ldc % 8 == 0
        for odt in (F32, dt):
            for kw in (dict(), dict(act=1), dict(add_mode="resid", ld_add=770), dict(add_mode=30, ld_add=776, add2_div=1, ld_add2=784),
                       dict(add_mode="alias", act=1)):
                if kw.get("add_mode") == "alias" and odt != F32:
                    continue                                       # (the addend is fp32: it can only alias an fp32 output)
                e = pc.gemm_abi_case(M, 768, 768, dt, lda=lda, ldc=ldc, out_dtype=odt, seed=M, **kw)
                dense_same = same and kw.get("ld_add", 768) % 8 == 0
                _check_plain(e, odt, K_GENERIC, f"small M={M} lda={lda} ldc={ldc} out={odt} {kw}", dense_same,
                             inplace=kw.get("add_mode") == "alias")


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("lda", [768, 776])
def test_generic_128_gemm_with_strides_that_rule_out_the_persistent_kernels(pc, tune, dt, lda):
    """Small-launch path off (SMALL_TILES = -1), 72 tiles: ldc = 772 (16-bit output, vector epilogue) and ld_add = 770 (fp32 output, scalar
    epilogue with N == N_pad) are not persistent_ok and not p256_eligible -> the generic 128 x 128 kernel."""
    tune("SMALL_TILES", -1)
    e = pc.gemm_abi_case(1409, 768, 768, dt, lda=lda, ldc=772, out_dtype=dt)
    _check_plain(e, dt, K_128, f"generic lda={lda} ldc=772 16-bit", False)
    e = pc.gemm_abi_case(1409, 768, 768, dt, lda=lda, ld_add=770, add_mode="resid", out_dtype=F32)
    _check_plain(e, F32, K_128, f"generic lda={lda} ld_add=770 fp32", False)
    e = pc.gemm_abi_case(1409, 768, 768, dt, lda=lda, ldc=770, act=1, out_dtype=F32)
    _check_plain(e, F32, K_128, f"generic lda={lda} ldc=770 fp32 relu", False)


def _check_fold(e, dt, kernel, what):
    print(f"{what}: vs_algebra {e['vs_algebra']:.3g} vs_layernorm {e['vs_layernorm']:.3g} kernels {e['kernels']} "
          f"bits equal to the dense call: {e['bits_equal']}")
    e["out"].assert_fully_written(what)
    e["out"].assert_untouched(what)
    assert e["kernels"] == [kernel], (what, e["kernels"])
    # test_gemm_layernorm_fold's bounds: output rounding of a 16-bit result / + operand rounding of x and gamma * W
    assert e["vs_algebra"] < (6e-3 if dt == BF16 else 8e-4) and e["vs_layernorm"] < (1.2e-2 if dt == BF16 else 1.6e-3), (what, e)
    assert e["bits_equal"], what


def _check_split(e, dt, kernel, what, inplace, stats):
    print(f"{what}: max_abs {e['max_abs']:.3g} kernels {e['kernels']} bits equal to the dense call: {e['bits_equal']}")
    for name in ("hi", "lo") + (("stats",) if stats else ()):
        if not inplace or name == "stats":
            e[name].assert_fully_written(f"{what} {name}")
        e[name].assert_untouched(f"{what} {name}")
    assert e["kernels"] == [kernel], (what, e["kernels"])
    assert e["res_intact"], what                                   # separate residual planes are inputs: not modified
    # test_gemm_split_residual_and_row_stats' bounds (same operands): hi + lo carries ~16 mantissa bits of values ~10
    assert e["max_abs"] < (2e-3 if dt == BF16 else 2e-4) and e["hi_is_rounding"], (what, e["max_abs"])
    if stats:
        assert e["stats_sum_err"] < 2e-3 and e["stats_sq_rel"] < 1e-4, (what, e["stats_sum_err"], e["stats_sq_rel"])
    assert e["bits_equal"], what


@pytest.mark.parametrize("dt", [BF16, F16])
def test_persistent_128_gemm_with_strides(pc, tune, dt):
    """SMALL_TILES = -1, P256_MODE = 2: the persistent 128 x 128 kernel, lda = ldc = 776, once per compiled epilogue mode."""
    tune("SMALL_TILES", -1)
    tune("P256_MODE", 2)
    e = pc.gemm_abi_case(1409, 768, 768, dt, lda=776, ldc=776, out_dtype=dt)
    _check_plain(e, dt, K_128, "persistent plain 16-bit", True)
    e = pc.gemm_abi_case(1409, 768, 768, dt, lda=776, ldc=776, out_dtype=F32, add_mode="resid", ld_add=772)
    _check_plain(e, F32, K_128, "persistent general fp32 + add", False)          # (ld_add 772 vs the dense call's 768: printed only)
    e = pc.gemm_abi_case(1409, 768, 768, dt, lda=776, ldc=776, out_dtype=F32, add_mode="alias")
    _check_plain(e, F32, K_128, "persistent general fp32, add aliases out", True, inplace=True)
    _check_fold(pc.gemm_fold_abi_case(1408, 768, dt, lda=776, ldc=776), dt, K_128, "persistent fold")
    _check_fold(pc.gemm_fold_abi_case(1408, 1024, dt, act=1, lda=776, ldc=1032), dt, K_128, "persistent fold + ReLU")
    tune("SPLIT_PIPE", 1)
    for inplace in (False, True):
        for stats in (True, False):
            e = pc.gemm_split_abi_case(1409, dt, lda=776, ldc=776, ld_res=784, inplace=inplace, want_stats=stats)
            _check_split(e, dt, K_128, f"persistent split inplace={inplace} stats={stats}", inplace, stats)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("K", [768, 1024])
def test_pipelined_split_gemm_with_strides(pc, tune, dt, K):
    """csrc/gemm_split.hip (SPLIT_PIPE = 0): split output + split residual + statistics + bias; its LDS-DMA loads build 32-bit byte
    offsets from lda.  Separate residual planes (ldc = 776, ld_res = 784) and the in-place form (ldc = ld_res = 776)."""
    tune("SMALL_TILES", -1)
    tune("P256_MODE", 2)
    lda = K + 8
    e = pc.gemm_split_abi_case(1409, dt, K=K, lda=lda, ldc=776, ld_res=784)
    _check_split(e, dt, K_SPLIT_PIPE, f"split pipe K={K} separate residual", False, True)
    e = pc.gemm_split_abi_case(1409, dt, K=K, lda=lda, ldc=776, inplace=True)
    _check_split(e, dt, K_SPLIT_PIPE, f"split pipe K={K} in place", True, True)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M", [256, 510, 1408])
def test_p256_gemm_with_strides(pc, tune, dt, M):
    """csrc/gemm_p256.hip alone (P256_MODE = 1): plain and LayerNorm fold with and without ReLU at N = 768 / 1024 / 2304, split output
    with and without statistics, in place and not; lda = 776, ldc = N + 8, ld_res = N + 16."""
    tune("SMALL_TILES", -1)
    tune("P256_MODE", 1)
    for N in (768, 1024, 2304):
        for act in (0, 1):
            e = pc.gemm_abi_case(M, N, 768, dt, lda=776, ldc=N + 8, act=act, out_dtype=dt, seed=N)
            _check_plain(e, dt, K_P256, f"p256 plain M={M} N={N} act={act}", True)
            _check_fold(pc.gemm_fold_abi_case(M, N, dt, act=act, lda=776, ldc=N + 8), dt, K_P256, f"p256 fold M={M} N={N} act={act}")
    for K in (768, 1024):
        for inplace in (False, True):
            for stats in (True, False):
                e = pc.gemm_split_abi_case(M, dt, K=K, lda=K + 8, ldc=776, ld_res=784, inplace=inplace, want_stats=stats)
                _check_split(e, dt, K_P256_SPLIT, f"p256 split M={M} K={K} inplace={inplace} stats={stats}", inplace, stats)


# ==== B. fp32 GEMM ("BG_F32: any shape") ============================================================================================
@pytest.mark.parametrize("M", [1, 5, 77])
@pytest.mark.parametrize("K", [1, 6, 7, 18, 768])
def test_gemm_fp32_any_shape_with_strides(pc, M, K):
    for N in (1, 6, 7, 768):
        for kw in (dict(), dict(act=1), dict(add_mode="resid", ld_add=N + 2), dict(add_mode=30, ld_add=N + 2, act=1), dict(add_mode="alias")):
            e = pc.gemm_abi_case(M, N, K, F32, lda=K + 3, ldc=N + 1, out_dtype=F32, seed=N, **kw)
            _check_plain(e, F32, K_F32, f"fp32 M={M} N={N} K={K} {kw}", False, inplace=kw.get("add_mode") == "alias")


# ==== C. attention ====================================================================================================================
ATTN_TOL = {BF16: (3e-2, 3e-3), F16: (4e-3, 4e-4), F32: (1e-5, 1e-5)}      # (max, mean): test_attention_bf16 / test_long_attention_kernel / _fp32


@pytest.mark.parametrize("dt", [BF16, F16, F32])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 64, 65, 130])
@pytest.mark.parametrize("mask", [None, "ragged", "one_empty"])
def test_attention_writes_every_row_and_nothing_else(pc, dt, N, mask):
    """B = 3 on each side of the N <= 32 / N <= 64 / long-kernel switches.  one_empty: every key of sample 1 is padded -- its rows are
    exactly 0 (brepgen_hip.h), the other samples stay within tolerance."""
    e = pc.attn_abi_case(3, N, dt, mask, seed=N)
    print(f"attention {dt} N={N} mask={mask}: max_abs {e['max_abs']:.3g} mean_abs {e['mean_abs']:.3g}")
    e["out"].assert_fully_written("attention out")
    e["out"].assert_untouched("attention out")
    assert e["finite"] and e["max_abs"] < ATTN_TOL[dt][0] and e["mean_abs"] < ATTN_TOL[dt][1], e["max_abs"]
    if mask == "one_empty":
        assert e["empty_rows_absmax"] == 0.0


@pytest.mark.parametrize("dt", [BF16, F16, F32])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 64, 65, 130])
def test_varlen_attention_leaves_rows_past_the_last_offset_alone(pc, dt, N):
    """bg_attn_varlen_fwd with offsets[B] < B * N: every kernel derives its row range from offsets[b] .. offsets[b + 1] - 1, so rows at
    and beyond offsets[B] are neither read nor written (brepgen_hip.h says so) -- they still hold the sentinel."""
    e = pc.attn_varlen_abi_case(3, N, dt, seed=N)
    print(f"varlen attention {dt} N={N}: {e['total']} of {3 * N} rows, max_abs {e['max_abs']:.3g}")
    e["out"].assert_untouched("varlen attention out")
    assert e["rows_below_all_written"] and e["rows_beyond_untouched"]
    assert e["max_abs"] < ATTN_TOL[dt][0], e["max_abs"]


# ==== D. element-wise and small kernels ==============================================================================================
def _guard(shape, dtype=F32, **kw):
    from guarded import guarded
    return guarded(shape, dtype, "cuda", **kw)


def _done(*gs, what=""):
    torch.cuda.synchronize()
    for i, g in enumerate(gs):
        g.assert_fully_written(f"{what} output {i}")
        g.assert_untouched(f"{what} output {i}")


@pytest.mark.parametrize("odt", [F32, BF16, F16])
@pytest.mark.parametrize("M", [1, 3, 61])
def test_layernorm_writes_its_rows_only(pc, odt, M):
    for silu in (False, True):
        out = _guard((M, 768), odt)
        e = pc.layernorm_case(M, odt, silu, out=out.view)
        _done(out, what=f"layernorm M={M} {odt} silu={silu}")
        # test_layernorm_fp32 / _bf16; fp16: the fp32 bound plus one rounding of the output to 11 significand bits
        tol = {F32: 5e-6, BF16: 2e-2 * max(1.0, e["ref_absmax"] / 4), F16: 5e-6 + 4.9e-4 * e["ref_absmax"]}[odt]
        assert e["finite"] and e["max_abs"] < tol, (silu, e["max_abs"])


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M", [1, 3, 130])
def test_layernorm_split_writes_its_rows_only(pc, dt, M):
    out = _guard((M, 768), dt)
    e = pc.layernorm_split_case(M, dt, out=out.view)
    _done(out, what=f"layernorm_split M={M}")
    assert e["finite"] and e["max_abs"] < (3e-2 if dt == BF16 else 4e-3)          # test_layernorm_split_input


@pytest.mark.parametrize("n", [1, 9])
def test_sincos_embed_writes_its_rows_only(pc, n):
    out = _guard((n, 768))
    e = pc.sincos_case((0, 1, 10, 249, 255, 500, 980, 995, 999)[-n:], out=out.view)
    _done(out, what=f"sincos n={n}")
    assert e["max_abs"] < 1e-4                                                      # test_sincos


def _ddpm_scalars(t=249):
    """DDPMScheduler.step's coefficients at step t of the 1000-step linear schedule, rounded to fp32 as the host does."""
    betas = torch.linspace(1e-4, 0.02, 1000, dtype=torch.float64)
    acp = torch.cumprod(1 - betas, 0)
    a_t, a_p = float(acp[t]), float(acp[t - 1])
    cur_a = a_t / a_p
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))
    var = (1 - a_p) / (1 - a_t) * (1 - cur_a)
    return dict(sa=f(math.sqrt(a_t)), sb=f(math.sqrt(1 - a_t)), x0c=f(math.sqrt(a_p) * (1 - cur_a) / (1 - a_t)),
                xtc=f(math.sqrt(cur_a) * (1 - a_p) / (1 - a_t)), sigma=f(math.sqrt(var)))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025])
def test_ddpm_step_writes_n_elements(pc, n):
    """The float4 path (n % 4 == 0) and the scalar one, with and without guidance / noise, against the kernel's formula restated in
    fp32 torch (same operations in the same order; the existing test's bounds: 1e-6, 2e-6 with guidance -- fma contraction)."""
    from brepgen_amd import _lib
    lib, c = _lib.load(), _ddpm_scalars()
    g = pc.gen(n)
    x = torch.randn(n, generator=g) * 1.5
    ec, eu, z = (torch.randn(n, generator=g) for _ in range(3))
    w = 0.6
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    for guided in (False, True):
        for noisy in (False, True):
            e = ec * (f32(1.0) + f32(w)) - eu * f32(w) if guided else ec
            x0 = ((x - f32(c["sb"]) * e) / f32(c["sa"])).clamp(-3.0, 3.0)
            want = f32(c["x0c"]) * x0 + f32(c["xtc"]) * x
            if noisy:
                want = want + f32(c["sigma"]) * z
            out = _guard(n)
            xd, ecd, eud, zd = x.cuda(), ec.cuda(), eu.cuda(), z.cuda()
            _lib.check(lib.bg_cfg_ddpm_step(ecd.data_ptr(), eud.data_ptr() if guided else None, w, xd.data_ptr(),
                                            zd.data_ptr() if noisy else None, out.view.data_ptr(), n, c["sa"], c["sb"], c["x0c"], c["xtc"],
                                            c["sigma"], 3.0, _lib.stream()), "bg_cfg_ddpm_step")
            _done(out, what=f"ddpm n={n} guided={guided} noisy={noisy}")
            err = float((out.view.cpu().reshape(-1) - want).abs().max())
            assert err <= (2e-6 if guided else 1e-6), (guided, noisy, err)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025])
def test_pndm_step_writes_n_elements(pc, n):
    """PRK phase 0 (e_store written, acc_out fresh), phases 1 / 2 (acc_out aliases acc, as schedulers.py runs them) and a PLMS step
    (e_store + three history tensors), guided and not; fp32 restatement, test_pndm_full_schedule's bounds (2e-6 / 4e-6 guided, x |ref|)."""
    from brepgen_amd import _lib
    lib = _lib.load()
    g = pc.gen(100 + n)
    x, ec, eu, acc, h0, h1, h2 = (torch.randn(n, generator=g) for _ in range(7))
    w = 0.6
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    sc, epc = 1.0123, 0.0456                                       # sample / eps coefficients of a mid-schedule step
    modes = [dict(name="prk0", store=True, acc=False, acc_out="fresh", so=0.0, se=1 / 6, ce=0.5, ca=0.0, hist=0),
             dict(name="prk1", store=False, acc=True, acc_out="alias", so=1.0, se=1 / 3, ce=0.5, ca=0.0, hist=0),
             dict(name="prk3", store=False, acc=True, acc_out=None, so=0.0, se=0.0, ce=1 / 6, ca=1.0, hist=0),
             dict(name="plms", store=True, acc=False, acc_out=None, so=0.0, se=0.0, ce=55 / 24, ca=0.0, hist=3)]
    for guided in (False, True):
        for m in modes:
            e = ec * (f32(1.0) + f32(w)) - eu * f32(w) if guided else ec
            comb = f32(m["ce"]) * e
            if m["ca"] != 0.0:
                comb = comb + f32(m["ca"]) * acc
            ch = (-59 / 24, 37 / 24, -9 / 24)
            for i, h in enumerate((h0, h1, h2)[:m["hist"]]):
                comb = comb + f32(ch[i]) * h
            want = f32(sc) * x - f32(epc) * comb
            want_acc = f32(m["so"]) * (acc if m["acc"] else torch.zeros(n)) + f32(m["se"]) * e
            out = _guard(n)
            store = _guard(n) if m["store"] else None
            acc_g = _guard(n)
            acc_g.view.copy_(acc.reshape(1, n))
            acc_out = acc_g if m["acc_out"] == "alias" else (_guard(n) if m["acc_out"] == "fresh" else None)
            dev = [t.cuda() for t in (x, ec, eu, h0, h1, h2)]
            p = lambda t: t.data_ptr() if t is not None else None
            _lib.check(lib.bg_pndm_step(p(dev[1]), p(dev[2]) if guided else None, w, p(dev[0]), p(store.view) if store else None,
                                        p(acc_g.view) if m["acc"] else None, p(acc_out.view) if acc_out else None, m["so"], m["se"],
                                        m["ce"], m["ca"], *[p(dev[3 + i]) if i < m["hist"] else None for i in range(3)],
                                        *ch, sc, epc, p(out.view), n, _lib.stream()), "bg_pndm_step")
            what = f"pndm n={n} {m['name']} guided={guided}"
            _done(*[b for b in (out, store, acc_g, acc_out) if b is not None and b is not acc_g] + [acc_g], what=what)
            tol = (4e-6 if guided else 2e-6)
            err = float((out.view.cpu().reshape(-1) - want).abs().max())
            assert err <= tol * max(1.0, float(want.abs().max())), (what, err)
            if store is not None:
                assert float((store.view.cpu().reshape(-1) - e).abs().max()) <= tol, what
            if acc_out is not None:
                assert float((acc_out.view.cpu().reshape(-1) - want_acc).abs().max()) <= tol * max(1.0, float(want_acc.abs().max())), what
            else:
                assert torch.equal(acc_g.view.cpu().reshape(-1), acc), what           # acc is an input there: unchanged


@pytest.mark.parametrize("per", [1, 5, 336])
def test_add_noise_writes_b_times_per_sample(pc, per):
    """out[b, :] = sa[b] * x0[b, :] + sb[b] * noise[b, :] (B = 3); the fp32 restatement differs from the kernel by an fma contraction at
    most: one ulp of |out| < 8, 9.5e-7 -> 1e-6."""
    from brepgen_amd import _lib
    g = pc.gen(per)
    B = 3
    x0, z = torch.randn(B, per, generator=g) * 1.5, torch.randn(B, per, generator=g)
    sa, sb = torch.rand(B, generator=g), torch.rand(B, generator=g)
    out = _guard((B, per))
    dev = [t.cuda() for t in (x0, z, sa, sb)]
    _lib.check(_lib.load().bg_add_noise(*[t.data_ptr() for t in dev], out.view.data_ptr(), B, per, _lib.stream()), "bg_add_noise")
    _done(out, what=f"add_noise per={per}")
    want = sa[:, None] * x0 + sb[:, None] * z
    assert float((out.view.cpu() - want).abs().max()) <= 1e-6


@pytest.mark.parametrize("per", [1, 3, 5, 48])
@pytest.mark.parametrize("raw", [1, 0])
def test_philox_tail_does_not_spill(pc, per, raw):
    """One Philox block yields 4 values: with per_sample % 4 != 0 the tail of a sample must stop at its own last element -- neither the
    next sample's first values nor the guard.  Bits / normals against oracle/philox.py as test_philox_bits_exact_and_normals_close."""
    import numpy as np
    from brepgen_amd import _lib
    from oracle import philox as ph
    n, seed, draw, first = 3, 0xC0FFEE1234567, 9, 1000
    out = _guard((n, per))
    _lib.check(_lib.load().bg_philox_randn(out.view.data_ptr(), n, per, seed, draw, first, raw, _lib.stream()), "bg_philox_randn")
    torch.cuda.synchronize()
    out.assert_untouched(f"philox per={per}")
    got = out.view.cpu().numpy()
    if raw:                                                         # (raw words may be any bit pattern: no `fully written` check on them)
        assert np.array_equal(got.view(np.uint32), ph.raw_bits(n, per, seed, draw, first))
    else:
        out.assert_fully_written(f"philox per={per}")
        assert np.abs(got - ph.randn(n, per, seed, draw, first)).max() < 2e-5


def test_masked_mse_writes_three_floats_and_1024_doubles(pc):
    from brepgen_amd import _lib
    g = pc.gen(8)
    rows, ld = 240, 18
    pred, tgt = torch.randn(rows, ld, generator=g), torch.randn(rows, ld, generator=g)
    mask = torch.rand(rows, generator=g) < 0.3
    pd, td, md = pred.cuda(), tgt.cuda(), mask.cuda().view(torch.uint8)
    for m, (c0, c1) in ((mask, (0, 18)), (None, (0, 18)), (mask, (0, 12)), (mask, (12, 18))):
        out3, scratch = _guard(3), _guard(1024, torch.float64)
        _lib.check(_lib.load().bg_masked_mse(pd.data_ptr(), td.data_ptr(), md.data_ptr() if m is not None else None, rows, ld, c0, c1 - c0,
                                             scratch.view.data_ptr(), out3.view.data_ptr(), _lib.stream()), "bg_masked_mse")
        _done(out3, scratch, what=f"masked_mse cols {c0}:{c1}")
        a, b = (pred, tgt) if m is None else (pred[~m], tgt[~m])
        a, b = a[:, c0:c1].double(), b[:, c0:c1].double()
        r = out3.view.cpu().reshape(-1)
        assert abs(float(r[0]) - float(((a - b) ** 2).mean())) < 1e-6               # test_masked_mse_matches_torch's bounds
        assert abs(float(r[1]) - float(((a - b) ** 2).mean(-1).sum())) < 1e-3
        assert int(r[2]) == a.shape[0]


@pytest.mark.parametrize("odt,tol", [(F32, 2e-5), (BF16, 2e-2), (F16, 3e-3)])
@pytest.mark.parametrize("rows", [1, 31, 33])
def test_embed_ln_silu_with_a_strided_poisoned_input(pc, odt, tol, rows):
    """k leading columns of rows that are lda = 18 floats apart (k = 48: lda = 51; lda < k is refused), everything else in x NaN."""
    from brepgen_amd import _lib
    for k in (6, 12, 48):
        lda = 18 if k <= 18 else k + 3
        out = _guard((rows, 768), odt)
        e = pc.embed_case(rows, k, odt, lda=lda, seed=rows + k, out=out.view, poison=True)
        _done(out, what=f"embed_ln_silu rows={rows} k={k}")
        assert e["finite"] and e["max_abs"] < tol, (k, e["max_abs"])                # test_embed_ln_silu_fp32 / _16bit_and_strided_input
    out = _guard((rows, 768), odt)
    with pytest.raises(_lib.BrepgenHipError, match=rf"code {_lib.BG_E_SHAPE}\)"):
        import hip_ops as ops
        x = torch.randn(rows * 3, 18, device="cuda")
        ops.embed_ln_silu(x.as_strided((rows, 48), (18, 1)), 48, torch.randn(768, 48, device="cuda"), *[torch.randn(768, device="cuda")] * 3,
                          out=out.view)
    torch.cuda.synchronize()
    assert not bool(out.written_mask().any())


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("rows", [1, 15, 17, 65])
def test_ln_silu_out_writes_a_tight_output(pc, dt, rows):
    for n_out in (1, 6, 18, 47, 48):
        out = _guard((rows, n_out))
        e = pc.ln_silu_out_case(rows, n_out, dt, out=out.view)
        _done(out, what=f"ln_silu_out rows={rows} n_out={n_out}")
        # test_ln_silu_out_vs_torch_fp32's bound
        assert e["finite"] and e["max_abs"] < (4e-3 if dt == BF16 else 6e-4) * max(1.0, e["ref_absmax"]), (n_out, e["max_abs"])


@pytest.mark.parametrize("dtype,tol", [(F32, 1e-5), (BF16, 3e-2), (F16, 4e-3)])
def test_embed_mlp_with_output_and_addend_strides(pc, dtype, tol):
    """bg_embed_mlp_fwd (z_embed: 48 -> 768 -> 768): x rows 51 floats apart with NaN between them, ldc = n_out + 3, a broadcast addend
    with ld_add = n_out + 5; test_encoder_layer_and_embed_mlp_entry_points' bounds."""
    from guarded import strided_input
    m, sd = pc.build_net("SurfZNet", 13, False, dtype)
    m.fold_layernorm = False
    w, _keep = m._pack(dtype)
    g = pc.gen(12)
    rows = 50
    z, add = torch.randn(rows, 48, generator=g), torch.randn(5, 768, generator=g)
    want = pc.orc.embed_mlp(sd, "z_embed", z)
    for with_add in (False, True):
        out = _guard((rows, 768), ld=771)
        kw = dict(add=strided_input(add.cuda(), 773), add_div=10, ld_add=773) if with_add else {}
        pc.ops.embed_mlp(w.embed[0], dtype, strided_input(z.cuda(), 51), out=out.view, ldc=771, **kw)
        _done(out, what=f"embed_mlp add={with_add}")
        ref = want + (add.repeat_interleave(10, 0) if with_add else 0)
        assert float((out.view.cpu() - ref).abs().max()) < tol * max(1.0, float(ref.abs().max()))


# ==== E. integer outputs =============================================================================================================
I32 = torch.int32


@pytest.mark.parametrize("B,n_mask,rep", [(1, 7, 1), (1, 7, 3), (5, 60, 1), (5, 9, 40)])
def test_compact_rows_leaves_entries_past_the_row_count_alone(pc, B, n_mask, rep):
    """offsets [B + 1] fully written; src_row [B * n_mask * rep]: the first offsets[B] entries written, `entries past offsets[B] are
    not written`.  B = 5: sample 1 has no valid token, sample 2 all n_mask of them."""
    from brepgen_amd import _lib
    g = pc.gen(B + n_mask)
    mask = torch.rand(B, n_mask, generator=g) < 0.45
    if B > 1:
        mask[1], mask[2] = True, False
    else:
        mask[0, 0], mask[0, 1] = False, True                       # (one valid, one padded at least)
    offs, src = _guard(B + 1, I32), _guard(B * n_mask * rep, I32)
    m_dev = mask.cuda().view(torch.uint8)
    _lib.check(_lib.load().bg_compact_rows(m_dev.data_ptr(), B, n_mask, rep, offs.view.data_ptr(), src.view.data_ptr(), _lib.stream()),
               "bg_compact_rows")
    _done(offs, what="compact_rows offsets")
    src.assert_untouched("compact_rows src_row")
    valid = (~mask).repeat_interleave(rep, dim=1)
    want_offs = torch.zeros(B + 1, dtype=torch.int64)
    want_offs[1:] = torch.cumsum(valid.sum(1), 0)
    total = int(want_offs[-1])
    assert 0 < total < B * n_mask * rep
    assert torch.equal(offs.view.cpu().reshape(-1).long(), want_offs)
    assert torch.equal(src.view.cpu().reshape(-1).long()[:total], torch.nonzero(valid.reshape(-1)).reshape(-1))
    written = src.written_mask().reshape(-1)
    assert bool(written[:total].all()) and not bool(written[total:].any())


@pytest.mark.parametrize("n", [[40], [0], [40, 0, 24, 39, 25], [64, 1, 63, 0, 17]])
def test_compact_rows_paired_writes_what_its_slots_need(pc, n):
    """Every output array guarded.  [40, 0, 24, 39, 25] (n_mask 40): a sample without a valid token, one of exactly n_mask tokens, two
    pairs whose lengths sum to exactly 64.  offsets and counts are written whole; slot_desc / slot_a up to the slot count and src_row
    up to offsets[B] = 64 x slots, nothing behind."""
    from brepgen_amd import _lib
    from test_gpu_round4 import _pair_slots_reference
    B, N = len(n), max(max(n), 1)
    mask = (torch.arange(N)[None] >= torch.tensor(n)[:, None])
    offs, src, sd, sa, cnt = _guard(B + 1, I32), _guard(64 * B, I32), _guard(2 * B, I32), _guard(B, I32), _guard(B, I32)
    m_dev = mask.to(torch.uint8).cuda()
    _lib.check(_lib.load().bg_compact_rows_paired(m_dev.data_ptr(), B, N, *[b.view.data_ptr() for b in (offs, src, sd, sa, cnt)], _lib.stream()),
               "bg_compact_rows_paired")
    _done(offs, cnt, what="compact_rows_paired offsets / counts")
    for b in (src, sd, sa):
        b.assert_untouched("compact_rows_paired")
    slots, start = _pair_slots_reference(n)
    ns = len(slots)
    offc, srcc, sdc, sac = (b.view.cpu().reshape(-1).tolist() for b in (offs, src, sd, sa))
    assert offc[B] == 64 * ns and cnt.view.cpu().reshape(-1).tolist() == n
    for k, (a, na, b, nb) in enumerate(slots):
        assert (sdc[2 * k], sdc[2 * k + 1], sac[k]) == (na, nb, a), k
        rows = [a * N + i for i in range(na)] + ([b * N + i for i in range(nb)] if b >= 0 else [])
        assert srcc[64 * k:64 * k + 64] == rows + [rows[0]] * (64 - len(rows)), k
    for b in range(B):
        assert offc[b] == (start[b] if n[b] > 0 else 0), b
    for buf, used in ((src, 64 * ns), (sd, 2 * ns), (sa, ns)):
        written = buf.written_mask().reshape(-1)
        assert bool(written[:used].all()) and not bool(written[used:].any())
    if n == [40, 0, 24, 39, 25]:
        assert sorted((na, nb) for _, na, _, nb in slots) == [(39, 25), (40, 24)]


@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("E", [1, 5])
def test_dedup_outputs_are_fully_written_and_nothing_else(pc, S, E):
    """bg_dedup_surfaces: pos_out `kept, 0-padded` and mask_out written whole; bg_dedup_edges: edge_mask written whole; results equal
    oracle/dedup.py (inputs as test_device_dedup_is_bit_identical_to_the_numpy_loops builds them)."""
    from brepgen_amd import _lib
    from oracle.dedup import dedup_edges_host, dedup_surfaces_host
    lib, B = _lib.load(), 2
    g = pc.gen(10 * S + E)
    base = torch.randn(B, 3, 6, generator=g).clamp(-3, 3)
    pos = torch.gather(base, 1, torch.randint(0, 3, (B, S), generator=g).unsqueeze(-1).expand(B, S, 6)).clone()
    pos = pos + (torch.rand(B, S, 6, generator=g) - 0.5) * 0.17
    hp, hm = dedup_surfaces_host(pos, 0.08)
    pos_out, mask_out = _guard((B, S, 6)), _guard((B, S), torch.uint8)
    pd = pos.cuda()
    thr = float(torch.tensor(0.08, dtype=torch.float32))
    _lib.check(lib.bg_dedup_surfaces(pd.data_ptr(), thr, pos_out.view.data_ptr(), mask_out.view.data_ptr(), B, S, _lib.stream()), "bg_dedup_surfaces")
    _done(pos_out, mask_out, what=f"dedup_surfaces S={S}")
    assert torch.equal(pos_out.view.cpu().reshape(B, S, 6), hp) and torch.equal(mask_out.view.cpu().reshape(B, S).bool(), hm)
    ebase = torch.randn(B, S, 2, 6, generator=g).clamp(-3, 3)
    ep = torch.gather(ebase, 2, torch.randint(0, 2, (B, S, E), generator=g).unsqueeze(-1).expand(B, S, E, 6)) + \
        (torch.rand(B, S, E, 6, generator=g) - 0.5) * 0.17
    odd = torch.zeros(B, S, dtype=torch.bool)
    odd[:, ::3] = S > 1                                              # a mask that is not left-aligned
    for sm in (hm, odd):
        em = _guard((B, S, E), torch.uint8)
        ed, sd_ = ep.cuda(), sm.to(torch.uint8).cuda()
        _lib.check(lib.bg_dedup_edges(ed.data_ptr(), sd_.data_ptr(), thr, em.view.data_ptr(), B, S, E, _lib.stream()), "bg_dedup_edges")
        _done(em, what=f"dedup_edges S={S} E={E}")
        assert torch.equal(em.view.cpu().reshape(B, S, E).bool(), dedup_edges_host(ep, sm, 0.08))


# ==== F. VAE leaf kernels (strides and guards; the numerics of the passes are tested elsewhere) ======================================
CODE = {F32: 0, F16: 1, BF16: 2}


def test_groupnorm_stats_writes_s_times_g_pairs(pc):
    """fp32 sums over 16 positions x 4 channels of values |x| < 5: n eps |x| = 64 x 6e-8 x 5 = 2e-5 on the mean, the same relative on rstd."""
    from brepgen_amd import _lib
    S, P, C, G = 2, 16, 64, 16
    x = torch.randn(S, P, C, generator=pc.gen(1)) * 1.3 + 0.4
    st = _guard((S, G, 2))
    xd = x.cuda()
    _lib.check(_lib.load().bg_groupnorm_stats(xd.data_ptr(), st.view.data_ptr(), S, P, C, G, 1e-6, _lib.stream()), "bg_groupnorm_stats")
    _done(st, what="groupnorm_stats")
    grp = x.double().reshape(S, P, G, C // G).permute(0, 2, 1, 3).reshape(S, G, -1)
    mean, rstd = grp.mean(-1), 1.0 / torch.sqrt(grp.var(-1, unbiased=False) + 1e-6)
    got = st.view.cpu().double().reshape(S, G, 2)
    assert float((got[..., 0] - mean).abs().max()) < 2e-5 and float(((got[..., 1] - rstd).abs() / rstd).max()) < 2e-5


def _im2col_ref(x, kh, kw, up, stride, pad_y, pad_x, Ho, Wo):
    """The gather of bg_im2col without normalisation, in plain indexing: x [S, H, W, C] -> [S * Ho * Wo, kh * kw * C], tap-major."""
    S, H, W, C = x.shape
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    H, W = x.shape[1], x.shape[2]
    need_h, need_w = (Ho - 1) * stride + kh, (Wo - 1) * stride + kw
    xp = torch.zeros(S, max(need_h, pad_y + H), max(need_w, pad_x + W), C, dtype=x.dtype)
    xp[:, pad_y:pad_y + H, pad_x:pad_x + W] = x
    out = torch.empty(S, Ho, Wo, kh, kw, C, dtype=x.dtype)
    for ky in range(kh):
        for kx in range(kw):
            out[:, :, :, ky, kx] = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
    return out.reshape(S * Ho * Wo, kh * kw * C)


@pytest.mark.parametrize("odt", [F32, BF16, F16])
def test_im2col_writes_its_matrix_only(pc, odt):
    """3 x 3 window on the plain and on the nearest-x2 up-sampled grid, stride 2 with Downsample2D's padding, and the 1 x 1 window with
    a residual: a gather (+ one fp32 add) -- exact; a 16-bit output is the rounding of that."""
    from brepgen_amd import _lib
    lib = _lib.load()
    S, H, W, C = 2, 4, 4, 64
    g = pc.gen(3)
    x = torch.randn(S, H, W, C, generator=g)
    add = torch.randn(S * H * W, C, generator=g)
    xd, addd = x.cuda(), add.cuda()
    for name, (kh, kw, up, stride, py, px, Ho, Wo, with_add) in dict(same=(3, 3, 0, 1, 1, 1, 4, 4, False), up=(3, 3, 1, 1, 1, 1, 8, 8, False),
                                                                     down=(3, 3, 0, 2, 0, 0, 2, 2, False), add=(1, 1, 0, 1, 0, 0, 4, 4, True)).items():
        out = _guard((S * Ho * Wo, kh * kw * C), odt)
        _lib.check(lib.bg_im2col(xd.data_ptr(), out.view.data_ptr(), CODE[odt], S, H, W, C, kh, kw, up, stride, py, px, Ho, Wo, None, None, None,
                                 1, 0, addd.data_ptr() if with_add else None, _lib.stream()), "bg_im2col")
        _done(out, what=f"im2col {name} {odt}")
        want = _im2col_ref(x, kh, kw, up, stride, py, px, Ho, Wo)
        if with_add:
            want = want + add
        assert torch.equal(out.view.cpu(), want.to(odt)), name


@pytest.mark.parametrize("L", [4, 16])
def test_cubic_resampling_writes_its_rows_only(pc, L):
    S, C = 3, 12
    up = _guard((S, 2 * L, C))
    e = pc.upsample1d_case(S, L, C, y=up.view.view(S, 2 * L, C))
    _done(up, what=f"upsample1d L={L}")
    assert e["max_abs"] < 1e-5                                      # test_gpu_round* bound for the same case
    down = _guard((S, L // 2, C))
    e = pc.downsample1d_case(S, L, C, y=down.view.view(S, L // 2, C))
    _done(down, what=f"downsample1d L={L}")
    assert e["max_abs"] < 1e-5


@pytest.mark.parametrize("odt", [BF16, F32])
@pytest.mark.parametrize("pad", [0, 1])
def test_small_attn_with_a_row_stride(pc, odt, pad):
    """ld = 3C (LDS-staged kernel) and ld = 3C + 1 (rows not 16-byte aligned: the unstaged kernel), the padding column NaN."""
    from brepgen_amd import _lib
    from guarded import strided_input
    S, T, C, nh = 5, 4, 512, 16
    qkv = torch.randn(S * T, 3 * C, generator=pc.gen(3))
    out = _guard((S * T, C), odt)
    scale = 1.0 / (C // nh) ** 0.5
    src = strided_input(qkv.cuda(), 3 * C + pad)
    _lib.check(_lib.load().bg_small_attn(src.data_ptr(), 3 * C + pad, out.view.data_ptr(), CODE[odt], S, T, C, nh, scale, _lib.stream()), "bg_small_attn")
    _done(out, what=f"small_attn ld=3C+{pad}")
    q, k, v = (t.double().reshape(S, T, nh, C // nh).transpose(1, 2) for t in qkv.split(C, dim=1))
    want = (torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v).transpose(1, 2).reshape(S * T, C)
    # test_small_attention_lds_image_is_padded_not_reordered's bounds
    assert float((out.view.cpu().double() - want).abs().max()) < (2e-2 if odt == BF16 else 2e-5)


@pytest.mark.parametrize("dt", [BF16, F16])
def test_conv_gemm_with_output_and_residual_strides(pc, dt):
    """The smallest problem with 64 tiles (S = 8, 32 x 32, C = 64, 3 x 3, N = 128): ldc = 136, a residual with ld_add = 132; and the
    narrow form (N = 3 real columns of a 128-row weight tile) with ldc = 3 and 4."""
    import ctypes
    from brepgen_amd import _lib
    from guarded import strided_input
    lib = _lib.load()
    S, H, W, C, kh, kw = 8, 32, 32, 64, 3, 3
    g = pc.gen(7)
    xn = torch.randn(S, H, W, C, generator=g).to(dt)
    w = (torch.randn(128, kh * kw * C, generator=g) * 0.05).to(dt)
    b = torch.randn(128, generator=g)
    add = torch.randn(S * H * W, 128, generator=g)
    xd, zero = xn.cuda(), torch.zeros(1 << 12, dtype=torch.uint8, device="cuda")

    def conv(N):
        return torch.nn.functional.conv2d(xn.float().permute(0, 3, 1, 2), w[:N].float().reshape(N, kh, kw, C).permute(0, 3, 1, 2), b[:N],
                                          padding=(kh // 2, kw // 2)).permute(0, 2, 3, 1).reshape(-1, N)

    for N, ldc, with_add in ((128, 136, False), (128, 136, True), (3, 3, False), (3, 4, False)):
        wN = w.clone()
        bN = b.clone()
        if N < 128:                                                 # narrow: weights and bias zero-padded to one 128-row tile
            wN[N:], bN[N:] = 0, 0
        wd, bd = wN.cuda(), bN.cuda()
        out = _guard((S * H * W, N), ld=ldc)
        addd = strided_input(add.cuda(), 132) if with_add else None
        d = _lib.ConvDesc()
        d.x, d.S, d.H, d.W, d.C = xd.data_ptr(), S, H, W, C
        d.kh, d.kw, d.up = kh, kw, 0
        d.w, d.bias, d.N = wd.data_ptr(), bd.data_ptr(), N
        d.out, d.ldc = out.view.data_ptr(), ldc
        d.add, d.ld_add = (addd.data_ptr(), 132) if with_add else (None, 0)
        d.dtype, d.zero_page = CODE[dt], zero.data_ptr()
        _lib.check(lib.bg_conv_gemm_fwd(ctypes.byref(d), _lib.stream()), "bg_conv_gemm_fwd")
        _done(out, what=f"conv_gemm N={N} ldc={ldc} add={with_add}")
        want = conv(N) + (add if with_add else 0)
        # test_narrow_convolution_as_implicit_gemm_equals_im2col_plus_generic_gemm's bound
        assert float((out.view.cpu() - want).abs().max()) < 2e-3 * max(1.0, float(want.abs().max())), (N, ldc)
