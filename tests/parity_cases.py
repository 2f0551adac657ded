"""Parity measurements: HIP path (through the C ABI) vs the CPU oracle / plain torch fp32 restatements.

Every function returns a dict of error metrics; ``tests/test_gpu_*.py`` assert on them and
``tests/gpu_check.py`` prints them all (one gpurun call gives the whole picture).  Needs a GPU.
"""
import json
import math
import os

import numpy as np
import torch

import brepgen_amd as bga
import hip_ops as ops
from oracle import denoisers as orc
from oracle.schedulers import OracleDDPM, OraclePNDM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"


def _err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    d = (got - want).abs()
    return {"max_abs": float(d.max()), "mean_abs": float(d.mean()), "ref_absmax": float(want.abs().max()),
            "finite": bool(torch.isfinite(got).all())}


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------
def layernorm_case(M, out_dtype, silu, seed=0, out=None):
    g = gen(seed)
    x = torch.randn(M, 768, generator=g) * 2 + 0.3
    w = 1 + 0.1 * torch.randn(768, generator=g)
    b = 0.1 * torch.randn(768, generator=g)
    want = torch.nn.functional.layer_norm(x.double(), (768,), w.double(), b.double(), 1e-5)
    if silu:
        want = torch.nn.functional.silu(want)
    got = ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), out_dtype=out_dtype, silu=silu, out=out)
    return _err(got.float(), want)


def sincos_case(t=(0, 1, 10, 249, 255, 500, 980, 995, 999), out=None):
    t = torch.tensor(list(t))
    return _err(ops.sincos_embed(t.to(DEV), out=out), orc.sincos_embedding(t))


def gemm_operands(M, N, K, dtype, n_valid=None, bias=True, add_mode=None, seed=0):
    """Seeded operands of gemm_case / gemm_abi_case on the CPU (a, w already rounded to `dtype`).
    add_mode: None | 'resid' (an [M, n_valid] addend, add_div = 1) | int d (broadcast rows m // d)."""
    g = gen(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bvec = torch.randn(N, generator=g) if bias else None
    nv = N if n_valid is None else n_valid
    add, add_div = None, 1
    if add_mode == "resid":
        add = torch.randn(M, nv, generator=g)
    elif isinstance(add_mode, int):
        add = torch.randn((M + add_mode - 1) // add_mode, nv, generator=g)
        add_div = add_mode
    return {"a": a.to(dtype), "w": w.to(dtype), "bias": bvec, "nv": nv, "add": add, "add_div": add_div, "gen": g}


def gemm_ref(o, act=0, add2=None, add2_div=1):
    """fp64 value of bg_gemm_bias_act_fwd / bg_gemm_ex_fwd's plain epilogue on the (already rounded) operands of gemm_operands."""
    M = o["a"].shape[0]
    ref = o["a"].double() @ o["w"].double().t()
    if o["bias"] is not None:
        ref = ref + o["bias"].double()
    if act:
        ref = ref.clamp_min(0)
    ref = ref[:, :o["nv"]]
    if o["add"] is not None:
        ref = ref + o["add"].double().repeat_interleave(o["add_div"], 0)[:M]
    if add2 is not None:
        ref = ref + add2.double().repeat_interleave(add2_div, 0)[:M]
    return ref


def gemm_case(M, N, K, dtype, n_valid=None, bias=True, act=0, add_mode=None, out_dtype=torch.float32, seed=0):
    """add_mode: None | 'resid' (in place, add_div=1) | int d (broadcast rows m//d)."""
    o = gemm_operands(M, N, K, dtype, n_valid, bias, add_mode, seed)
    ref = gemm_ref(o, act)
    out, add_t = None, None
    if add_mode == "resid":
        out = o["add"].clone().to(DEV)
        add_t = out
    elif o["add"] is not None:
        add_t = o["add"].to(DEV)
    got = ops.linear(o["a"].to(DEV), o["w"].to(DEV), o["bias"].to(DEV) if bias else None, out_dtype=out_dtype, act=act,
                     add=add_t, add_div=o["add_div"], n_valid=o["nv"], out=out)
    return _err(got.float(), ref)


def _attn_ref(qkv, mask, B, N):
    """fp64 reference on the (already rounded) operands; q is pre-scaled."""
    q, k, v = qkv.double().reshape(B, N, 3, 12, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask.reshape(B, 1, 1, N), float("-inf"))
    p = torch.softmax(s, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * N, 768)


def attn_case(B, N, dtype, mask_kind="ragged", seed=0, scale=1.0):
    g = gen(seed)
    qkv = torch.randn(B * N, 2304, generator=g) * scale
    qkv[:, :768] *= 0.125 * 2.0          # pre-scaled q, with some spread in the logits
    mask = None
    if mask_kind == "ragged":
        mask = torch.ones(B, N, dtype=torch.bool)
        for b in range(B):
            mask[b, : int(torch.randint(1, N + 1, (1,), generator=g))] = False
    elif mask_kind == "random":
        mask = torch.rand(B, N, generator=g) < 0.5
        mask[:, 0] = False
    qd = qkv.to(dtype)
    want = _attn_ref(qd, mask, B, N)
    got = ops.attention(qd.to(DEV), mask.to(DEV) if mask is not None else None, B, N)
    return _err(got.float(), want)


# ---------------------------------------------------------------------------------------------------
def ddpm_case(t, shape=(4, 60, 48), guidance=None, clip=True, seed=0):
    g = gen(seed)
    x = torch.randn(*shape, generator=g) * 1.5
    B = shape[0]
    eps = torch.randn(*((2 * B,) + shape[1:]) if guidance else shape, generator=g)
    noise = torch.randn(*shape, generator=g)
    o = OracleDDPM(clip_sample=clip, clip_sample_range=3)
    o.set_timesteps(1000)
    s = bga.DDPMScheduler(num_train_timesteps=1000, beta_schedule="linear", prediction_type="epsilon",
                          beta_start=0.0001, beta_end=0.02, clip_sample=clip, clip_sample_range=3)
    s.set_timesteps(1000)
    e_eff = eps if not guidance else eps[:B] * (1 + guidance) - eps[B:] * guidance
    want = o.step(e_eff, t, x, noise=noise)
    got = s.step(eps.to(DEV), torch.tensor(t), x.to(DEV), noise=noise.to(DEV), guidance=guidance).prev_sample
    return _err(got, want)


def pndm_case(n_steps=209, shape=(3, 30, 6), guidance=None, seed=0):
    """Drive both PNDM implementations with the same pseudo-model eps = f(x, t) and compare every step."""
    g = gen(seed)
    x0 = torch.randn(*shape, generator=g)
    B = shape[0]
    o = OraclePNDM()
    o.set_timesteps(200)
    s = bga.PNDMScheduler(num_train_timesteps=1000, beta_schedule="linear", prediction_type="epsilon",
                          beta_start=0.0001, beta_end=0.02)
    s.set_timesteps(200)
    assert s.timesteps.tolist() == o.timesteps.tolist()
    xo, xs = x0.clone(), x0.clone().to(DEV)
    worst = 0.0
    for i, t in enumerate(s.timesteps[:n_steps]):
        noise_like = torch.randn(*((2 * B,) + shape[1:]) if guidance else shape, generator=g)
        # pseudo network: depends on the current sample so errors would propagate
        def net(x):
            rep = x.repeat(2, *([1] * (x.dim() - 1))) if guidance else x
            return 0.5 * torch.tanh(rep) + 0.3 * noise_like.to(x.device)
        eo = net(xo)
        if guidance:
            eo = eo[:B] * (1 + guidance) - eo[B:] * guidance
        xo = o.step(eo, t, xo)
        xs = s.step(net(xs), t, xs, guidance=guidance).prev_sample
        worst = max(worst, float((xs.cpu() - xo).abs().max()))
    return {"max_abs": worst, "ref_absmax": float(xo.abs().max()), "finite": bool(torch.isfinite(xs).all()),
            "mean_abs": worst}


def embed_case(rows, k, out_dtype, lda=None, col0=0, seed=0, out=None, poison=False):
    """Fused Linear(k) + LayerNorm + SiLU vs plain torch fp64 math.  poison: the columns of x outside [col0, col0 + k) hold NaN."""
    g = gen(seed)
    lda = lda or k
    xfull = torch.randn(rows, lda, generator=g) * 1.5
    w0, b0 = torch.randn(768, k, generator=g) * 0.3, torch.randn(768, generator=g) * 0.1
    gamma, beta = 1 + 0.1 * torch.randn(768, generator=g), 0.1 * torch.randn(768, generator=g)
    xd = xfull.to(DEV)
    if poison:
        keep = torch.zeros(lda, dtype=torch.bool)
        keep[col0:col0 + k] = True
        xd[:, ~keep.to(DEV)] = float("nan")
    got = ops.embed_ln_silu(xd[:, col0:], k, w0.to(DEV), b0.to(DEV), gamma.to(DEV), beta.to(DEV), out_dtype, out=out)
    x = xfull[:, col0:col0 + k].double()
    h = torch.nn.functional.layer_norm(x @ w0.double().t() + b0.double(), (768,), gamma.double(), beta.double(), 1e-5)
    return _err(got.float(), torch.nn.functional.silu(h).float())


def _split(x, dt):
    hi = x.to(dt)
    return hi, (x - hi.float()).to(dt)


def split_operands(M, dtype, K=768, N=768, seed=0):
    """Seeded operands of the split-residual producer epilogue (CPU): a, w, bias, the fp32 residual x and its planes hi + lo."""
    g = gen(seed)
    a = (torch.randn(M, K, generator=g) * 0.5).to(dtype)
    w = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    bias = torch.randn(N, generator=g)
    x = torch.randn(M, N, generator=g) * 3 + 0.7
    hi, lo = _split(x, dtype)
    return {"a": a, "w": w, "bias": bias, "x": x, "hi": hi, "lo": lo}


def split_metrics(o, dtype, out_hi, out_lo, stats, with_res=True):
    """Error metrics of a split-output launch on split_operands `o` vs fp64: the planes' sum, hi being the rounding of the value, and
    (stats given) the per-64-column row statistics [N/64, M, 2]."""
    a, w = o["a"], o["w"]
    M, N = a.shape[0], w.shape[0]
    want = a.double() @ w.double().t() + o["bias"].double() + ((o["hi"].double() + o["lo"].double()) if with_res else o["x"].double())
    got = out_hi.double().cpu() + out_lo.double().cpu()
    e = {"max_abs": float((got - want).abs().max()),
         "hi_is_rounding": bool((out_hi.cpu().float() - want.float().to(dtype).float()).abs().max() <= 2 * float(want.abs().max()) * 2 ** -8)}
    if stats is not None:
        st = stats.double().cpu().reshape(N // 64, M, 2).permute(1, 0, 2)      # part-major on the device
        grp = want.reshape(M, N // 64, 64)
        e["stats_sum_err"] = float((st[..., 0] - grp.sum(-1)).abs().max())
        e["stats_sq_rel"] = float(((st[..., 1] - (grp * grp).sum(-1)).abs() / (grp * grp).sum(-1)).max())
    return e


def gemm_split_case(M, dtype, K=768, N=768, with_res=True, seed=0):
    """Split-residual producer epilogue: hi/lo planes + per-64-column row statistics vs plain torch fp32 math."""
    o = split_operands(M, dtype, K, N, seed)
    kw = dict(res=(o["hi"].to(DEV), o["lo"].to(DEV))) if with_res else dict(add=o["x"].to(DEV))
    r = ops.linear_ex(o["a"].to(DEV), o["w"].to(DEV), o["bias"].to(DEV), split_out=True, want_stats=True, **kw)
    e = split_metrics(o, dtype, r["out"], r["lo"], r["stats"], with_res)
    e.update(hi=r["out"], lo=r["lo"], stats=r["stats"])
    return e


def fold_operands(M, N, dtype, seed=0):
    """Seeded operands of the LayerNorm-fold consumer epilogue (CPU)."""
    g = gen(seed)
    K = 768
    x = torch.randn(M, K, generator=g) * 2.5 + torch.randn(M, 1, generator=g)      # per-row mean up to ~1 sigma/2
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    W, b = torch.randn(N, K, generator=g) * 0.04, torch.randn(N, generator=g) * 0.1
    hi, _ = _split(x, dtype)
    grp = x.reshape(M, K // 64, 64)
    stats = torch.stack([grp.sum(-1), (grp * grp).sum(-1)], -1).permute(1, 0, 2).contiguous()    # [12, M, 2]
    Wp = (W * gamma[None]).to(dtype)
    return {"x": x, "gamma": gamma, "beta": beta, "W": W, "b": b, "hi": hi, "stats": stats, "Wp": Wp,
            "colsum": Wp.float().sum(1), "c": b + W @ beta}


def fold_metrics(o, out, act=0):
    """A fold launch's output on fold_operands `o` vs (a) the same algebra in fp64 and (b) LayerNorm(x) @ W^T + b itself, both relative
    to max |y|."""
    x, hi, Wp, colsum, c = o["x"], o["hi"], o["Wp"], o["colsum"], o["c"]
    got = out.double().cpu()
    mean = x.double().mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.double().var(-1, unbiased=False, keepdim=True) + 1e-5)
    alg = rstd * (hi.double() @ Wp.double().t()) - mean * rstd * colsum.double()[None] + c.double()[None]
    ln = ((x.double() - mean) * rstd * o["gamma"].double() + o["beta"].double()) @ o["W"].double().t() + o["b"].double()
    if act:
        alg, ln = alg.clamp(min=0), ln.clamp(min=0)
    scale = float(ln.abs().max())
    return {"vs_algebra": float((got - alg).abs().max()) / scale, "vs_layernorm": float((got - ln).abs().max()) / scale}


def gemm_fold_case(M, N, dtype, act=0, seed=0):
    """LayerNorm-fold consumer epilogue vs (a) the same algebra in fp64 and (b) LayerNorm(x) @ W^T + b itself."""
    o = fold_operands(M, N, dtype, seed)
    r = ops.linear_ex(o["hi"].to(DEV), o["Wp"].to(DEV), o["c"].to(DEV), act=act, stats_in=o["stats"].to(DEV),
                      colsum=o["colsum"].to(DEV))
    e = fold_metrics(o, r["out"], act)
    e["out"] = r["out"]
    return e


def layernorm_split_case(M, dtype, seed=0, out=None):
    g = gen(seed)
    x = torch.randn(M, 768, generator=g) * 2 + 0.3
    hi, lo = _split(x, dtype)
    gamma, beta = 1 + 0.1 * torch.randn(768, generator=g), 0.1 * torch.randn(768, generator=g)
    got = ops.layernorm_split(hi.to(DEV), lo.to(DEV), gamma.to(DEV), beta.to(DEV), out=out)
    want = torch.nn.functional.layer_norm(hi.float() + lo.float(), (768,), gamma, beta, 1e-5)
    return _err(got.float(), want)


# ---------------------------------------------------------------------------------------------------
NETS = {"SurfPosNet": bga.SurfPosNet, "SurfZNet": bga.SurfZNet, "EdgePosNet": bga.EdgePosNet, "EdgeZNet": bga.EdgeZNet}
MANIFEST = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))


def build_net(net, seed, use_cf, dtype, varlen=False, weights="seeded"):
    """varlen=False: dense execution (every position as the reference computes it) -- what the position-exact parity
    tests check; varlen=True: the product default (valid tokens only, 0 at padded positions)."""
    sd = orc.make_state_dict(weights, net, seed, use_cf)
    m = NETS[net](use_cf)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    m.compute_dtype = dtype
    m.varlen = varlen
    return m, sd


def golden_case(name, dtype, varlen=False, fold=True, center=True, autocast_ref=False):
    """HIP denoiser vs the golden output written by the reference's own class (tests/golden/gen_golden.py).
    autocast_ref: also run oracle/ref_formulation.py (the reference's formulation: stock nn.TransformerEncoder) under
    torch.autocast('cuda', dtype) on the same inputs -- how sample.py:121 runs the reference -- and report its error."""
    meta = MANIFEST["cases"][name]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    args = [torch.from_numpy(z[k]).to(DEV) if k in z.files else None for k in meta["args"]]
    m, sd = build_net(meta["net"], meta["weight_seed"], meta["use_cf"], dtype, varlen, meta.get("weights", "seeded"))
    m.fold_layernorm, m.center_stream = fold, center
    with torch.no_grad():
        got = m(*args)
    want = torch.from_numpy(z["out"])
    e = _err(got, want)
    e["got"] = got.cpu()
    mk = "surf_mask" if "surf_mask" in meta["args"] else ("mask" if "mask" in meta["args"] else None)
    vsel = ~torch.from_numpy(z[mk]) if mk is not None else torch.ones(want.shape[:-1], dtype=torch.bool)
    if meta["net"] == "EdgePosNet" and mk is not None:
        vsel = vsel.unsqueeze(-1).expand(want.shape[:-1])
    e["mean_abs_valid"] = float((got.cpu() - want)[vsel].abs().mean())
    if autocast_ref:
        from oracle import ref_formulation as rf
        ref = rf.build(meta["net"], sd, meta["use_cf"]).to(DEV)
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
            ra = ref(*args).float().cpu()
        e["autocast_max_abs_valid"] = float((ra - want)[vsel].abs().max())
        e["autocast_mean_abs_valid"] = float((ra - want)[vsel].abs().mean())
    mask_key = "surf_mask" if "surf_mask" in meta["args"] else ("mask" if "mask" in meta["args"] else None)
    if mask_key is not None and meta["net"] != "EdgePosNet":
        valid = ~torch.from_numpy(z[mask_key])
        e["max_abs_valid"] = float((got.cpu() - want)[valid].abs().max())
    elif mask_key is not None:
        valid = ~torch.from_numpy(z[mask_key])
        e["max_abs_valid"] = float((got.cpu() - want)[valid].abs().max())
    else:
        e["max_abs_valid"] = e["max_abs"]
    return e


def synth_inputs(net, B, S, E, use_cf, seed=1234):
    """Synthetic DeepCAD-shaped inputs per SURVEY.md section 8(d)."""
    g = gen(seed)
    R = lambda *s: torch.randn(*s, generator=g)
    t = torch.tensor([249])
    cl = None
    if use_cf:
        cl = torch.cat([torch.full((B // 2, 1), 6), torch.zeros(B - B // 2, 1, dtype=torch.long)]).long()
    smask = torch.ones(B, S, dtype=torch.bool)
    for b in range(B):
        smask[b, : int(torch.randint(min(8, S), S + 1, (1,), generator=g))] = False
    if net == "SurfPosNet":
        return [R(B, S, 6).clamp(-3, 3), t, cl]
    if net == "SurfZNet":
        return [R(B, S, 48), t, R(B, S, 6).clamp(-3, 3), smask, cl]
    if net == "EdgePosNet":
        return [R(B, S, E, 6).clamp(-3, 3), t, R(B, S, 6).clamp(-3, 3), R(B, S, 48), smask, cl]
    em = torch.rand(B, S, E, generator=g) < 0.4
    em[:, :, 0] = False
    em = em | smask.unsqueeze(-1)
    em[:, 0, 0] = False
    return [R(B, S, E, 18), t, R(B, S, E, 6).clamp(-3, 3), R(B, S, 6).clamp(-3, 3), R(B, S, 48), em, cl]


def oracle_case(net, B, S, E, dtype, use_cf=False, seed=7, varlen=False):
    """HIP denoiser vs the CPU oracle on seeded inputs at a size the oracle finishes in seconds."""
    m, sd = build_net(net, seed, use_cf, dtype, varlen)
    args = synth_inputs(net, B, S, E, use_cf)
    with torch.no_grad():
        want = orc.FORWARD[net](sd, *args)
        got = m(*[a.to(DEV) if torch.is_tensor(a) else a for a in args])
    e = _err(got, want)
    mask = args[3] if net == "SurfZNet" else (args[4] if net == "EdgePosNet" else (args[5] if net == "EdgeZNet" else None))
    if mask is not None:
        valid = ~mask if net != "EdgePosNet" else (~mask)[:, :, None].expand(B, S, E)
        e["max_abs_valid"] = float((got.cpu() - want)[valid].abs().max())
        e["padded_absmax"] = float(got.cpu()[~valid].abs().max()) if bool((~valid).any()) else 0.0
    else:
        e["max_abs_valid"] = e["max_abs"]
        e["padded_absmax"] = 0.0
    return e


_SD_DEV = {}


def oracle_on_device(fn, sd, *args):
    """The fp32 oracle forward `fn(sd, *args)` evaluated on the GPU (plain torch; gfx950 has no TF32) and returned on the CPU:
    the chain / cascade tests call the oracle hundreds of times on tiny batches, which costs ~0.2 s per call on the host."""
    key = id(sd)
    if key not in _SD_DEV:
        _SD_DEV[key] = ({k: v.to(DEV) for k, v in sd.items()}, sd)      # (keep sd alive: the cache is keyed on its id)
    mv = lambda a: a.to(DEV) if torch.is_tensor(a) else a
    with torch.no_grad():
        return fn(_SD_DEV[key][0], *[mv(a) for a in args]).cpu()


def ddpm_chain_case(dtype, steps=50, B=1, N=60, seed=3, last=None, oracle_dev=True):
    """BASELINE configs[0]: B=1 face-LDM, `steps` DDPM steps of SurfZNet with injected noise, HIP vs oracle.
    Both chains are fed the ORACLE's trajectory (per-step parity: same x_t in, compare x_{t-1} out)."""
    m, sd = build_net("SurfZNet", seed, False, dtype)
    g = gen(99)
    surfPos = torch.randn(B, N, 6, generator=g).clamp(-3, 3)
    mask = torch.zeros(B, N, dtype=torch.bool)
    mask[:, 40:] = True
    x = torch.randn(B, N, 48, generator=g)
    o = OracleDDPM(clip_sample=True, clip_sample_range=3)
    o.set_timesteps(steps)
    s = bga.DDPMScheduler(num_train_timesteps=1000, beta_schedule="linear", prediction_type="epsilon",
                          beta_start=0.0001, beta_end=0.02, clip_sample=True, clip_sample_range=3)
    s.set_timesteps(steps)
    worst_eps = worst_x = 0.0
    sp_d, mk_d = surfPos.to(DEV), mask.to(DEV)
    with torch.no_grad():
        for t in (s.timesteps if last is None else s.timesteps[-last:]):
            noise = torch.randn(B, N, 48, generator=g)
            tt = t.reshape(-1)
            eo = oracle_on_device(orc.surfz_forward, sd, x, tt, surfPos, mask) if oracle_dev else orc.surfz_forward(sd, x, tt, surfPos, mask)
            xo = o.step(eo, t, x, noise=noise)
            eh = m(x.to(DEV), tt.to(DEV), sp_d, mk_d, None)
            xh = s.step(eh, t, x.to(DEV), noise=noise.to(DEV)).prev_sample
            worst_eps = max(worst_eps, float((eh.cpu() - eo)[~mask].abs().max()))
            worst_x = max(worst_x, float((xh.cpu() - xo)[~mask].abs().max()))
            x = xo
    return {"max_abs_eps": worst_eps, "max_abs_x": worst_x, "finite": bool(torch.isfinite(xh).all())}


# ---------------------------------------------------------------------------------------------------
SURF_CFG = dict(in_channels=3, out_channels=3, down_block_types=["DownEncoderBlock2D"] * 4,
                up_block_types=["UpDecoderBlock2D"] * 4, block_out_channels=[128, 256, 512, 512], layers_per_block=2,
                act_fn="silu", latent_channels=3, norm_num_groups=32, sample_size=512)          # sample.py:72-82
EDGE_CFG = dict(in_channels=3, out_channels=3, down_block_types=["DownBlock1D"] * 3, up_block_types=["UpBlock1D"] * 3,
                block_out_channels=[128, 256, 512], layers_per_block=2, act_fn="silu", latent_channels=3,
                norm_num_groups=32, sample_size=512)                                            # sample.py:86-97


def vae_case(kind, n, dtype, seed=0):
    """HIP VAE decoder vs the oracle restatement (oracle/vae.py) on seeded weights and latents."""
    from oracle import vae as ov
    g = gen(100 + seed)
    if kind == "surf":
        sd = ov.seeded_state_dict(ov.surf_decoder_spec(), 31 + seed)
        m = bga.AutoencoderKLFastDecode(**SURF_CFG)
        z = torch.randn(n, 3, 4, 4, generator=g)
        with torch.no_grad():
            want = ov.surf_decode(sd, z)
    elif kind == "surf_enc":
        sd = ov.seeded_state_dict(ov.surf_encoder_spec(), 51 + seed)
        m = bga.AutoencoderKLFastEncode(**SURF_CFG)
        z = torch.randn(n, 3, 32, 32, generator=g)
        with torch.no_grad():
            want = ov.surf_encode(sd, z)
    elif kind == "edge_enc":
        sd = ov.seeded_state_dict(ov.edge_encoder_spec(), 61 + seed)
        m = bga.AutoencoderKL1DFastEncode(**EDGE_CFG)
        z = torch.randn(n, 3, 32, generator=g)
        with torch.no_grad():
            want = ov.edge_encode(sd, z)
    else:
        sd = ov.seeded_state_dict(ov.edge_decoder_spec(), 41 + seed)
        m = bga.AutoencoderKL1DFastDecode(**EDGE_CFG)
        z = torch.randn(n, 3, 4, generator=g)
        with torch.no_grad():
            want = ov.edge_decode(sd, z)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    m.compute_dtype = dtype
    with torch.no_grad():
        got = m(z.to(DEV))
    assert got.shape == want.shape
    return _err(got, want)


def upsample1d_case(S=3, L=8, C=12, y=None):
    from oracle import vae as ov
    from brepgen_amd import _lib
    g = gen(5)
    x = torch.randn(S, C, L, generator=g)
    want = ov.upsample1d_cubic(x)                                  # [S, C, 2L]
    xc = x.permute(0, 2, 1).contiguous().to(DEV)
    y = torch.empty(S, 2 * L, C, device=DEV) if y is None else y
    _lib.check(_lib.load().bg_upsample1d_cubic(xc.data_ptr(), y.data_ptr(), S, L, C, _lib.stream()), "upsample")
    return _err(y.permute(0, 2, 1), want)


def downsample1d_case(S=3, L=16, C=12, y=None):
    from oracle import vae as ov
    from brepgen_amd import _lib
    g = gen(6)
    x = torch.randn(S, C, L, generator=g)
    want = ov.downsample1d_cubic(x)
    xc = x.permute(0, 2, 1).contiguous().to(DEV)
    y = torch.empty(S, L // 2, C, device=DEV) if y is None else y
    _lib.check(_lib.load().bg_downsample1d_cubic(xc.data_ptr(), y.data_ptr(), S, L, C, _lib.stream()), "downsample")
    return _err(y.permute(0, 2, 1), want)


# ---------------------------------------------------------------------------------------------------
# Stride-aware variants for tests/test_gpu_abi_contract.py: the same operands and fp64 references as above, called with explicit row
# strides on guard-banded, sentinel-filled buffers (tests/guarded.py) and once more the ordinary way (dense tensors) for the bit
# comparison.  Every function returns the Guarded outputs, so that the test asserts "everything written, nothing else touched".
def profiled(fn):
    """(fn(), [kernel name of every profiler row]) -- bg_profile_begin / bg_profile_end around fn: which kernels served the call."""
    from brepgen_amd import _lib
    with _lib.profile(16) as p:
        r = fn()
    return r, [row["kernel"] for row in p.rows if row["launches"] > 0]


def gemm_abi_case(M, N, K, dtype, *, n_valid=None, lda=None, ldc=None, ld_add=None, ld_add2=None, act=0, out_dtype=torch.float32,
                  add_mode=None, add2_div=None, seed=0):
    """bg_gemm_bias_act_fwd (bg_gemm_ex_fwd with add2_div) with explicit strides on a guarded output.
    add_mode: None | 'resid' ([M, n] addend, row stride ld_add) | 'alias' (the addend IS the output buffer, in place) | int d
    (broadcast rows m // d, row stride ld_add).  add2_div: a second addend [ceil(M / d), n] with row stride ld_add2."""
    from guarded import guarded, strided_input
    o = gemm_operands(M, N, K, dtype, n_valid, True, "resid" if add_mode == "alias" else add_mode, seed)
    nv = o["nv"]
    add2 = torch.randn((M + add2_div - 1) // add2_div, nv, generator=o["gen"]) if add2_div else None
    ref = gemm_ref(o, act, add2, add2_div or 1)
    a_d, w_d, b_d = o["a"].to(DEV), o["w"].to(DEV), o["bias"].to(DEV)
    add_d = o["add"].to(DEV) if o["add"] is not None else None
    add2_d = add2.to(DEV) if add2 is not None else None
    lda, ldc = lda or K, ldc or nv
    a_in = strided_input(a_d, lda) if lda != K else a_d
    out = guarded((M, nv), out_dtype, DEV, ld=ldc)
    add_in = None
    if add_mode == "alias":
        out.view.copy_(add_d)
        add_in, ld_add = out.view, ldc
    elif add_d is not None:
        ld_add = ld_add or nv
        add_in = strided_input(add_d, ld_add)
    add2_in = strided_input(add2_d, ld_add2 or nv) if add2_d is not None else None

    def call(a, out_t, add, add2_t, **ld):
        if add2_t is None:
            return ops.linear(a, w_d, b_d, act=act, add=add, add_div=o["add_div"], n_valid=nv, out=out_t, **ld)
        return ops.linear_ex(a, w_d, b_d, act=act, out_dtype=out_dtype, add=add, add_div=o["add_div"], add2=add2_t, add2_div=add2_div,
                             out=out_t, **ld)["out"]

    ld = dict(lda=lda, ldc=ldc, ld_add=ld_add if add_in is not None else None)
    if add2_in is not None:
        ld["ld_add2"] = ld_add2 or nv
    _, kernels = profiled(lambda: call(a_in, out.view, add_in, add2_in, **ld))
    dense = add_d.clone() if add_mode == "alias" else torch.empty(M, nv, device=DEV, dtype=out_dtype)
    call(a_d, dense, dense if add_mode == "alias" else add_d, add2_d)
    torch.cuda.synchronize()
    e = _err(out.view.float(), ref)
    e.update(out=out, kernels=kernels, bits_equal=bool(torch.equal(out.view, dense)))
    return e


def gemm_fold_abi_case(M, N, dtype, act=0, lda=None, ldc=None, seed=0):
    """LayerNorm-fold launch (bg_gemm_ex_fwd, stats_in / colsum) with a strided A and a guarded, strided output."""
    from guarded import guarded, strided_input
    o = fold_operands(M, N, dtype, seed)
    hi, Wp, c, st, cs = (o[k].to(DEV) for k in ("hi", "Wp", "c", "stats", "colsum"))
    lda, ldc = lda or 768, ldc or N
    out = guarded((M, N), dtype, DEV, ld=ldc)
    a_in = strided_input(hi, lda) if lda != 768 else hi
    _, kernels = profiled(lambda: ops.linear_ex(a_in, Wp, c, act=act, stats_in=st, colsum=cs, lda=lda, ldc=ldc, out=out.view))
    dense = ops.linear_ex(hi, Wp, c, act=act, stats_in=st, colsum=cs)["out"]
    torch.cuda.synchronize()
    e = fold_metrics(o, out.view, act)
    e.update(out=out, kernels=kernels, bits_equal=bool(torch.equal(out.view, dense)))
    return e


def gemm_split_abi_case(M, dtype, K=768, N=768, *, lda=None, ldc=None, ld_res=None, inplace=False, want_stats=True, seed=0):
    """Split-output launch with a split residual: out / out_lo / stats_out guarded; the residual planes either separate strided
    buffers (row stride ld_res) or the output planes themselves (inplace: ld_res = ldc)."""
    from guarded import guarded, strided_input
    o = split_operands(M, dtype, K, N, seed)
    a, w, b, hi, lo = (o[k].to(DEV) for k in ("a", "w", "bias", "hi", "lo"))
    lda, ldc = lda or K, ldc or N
    ld_res = ldc if inplace else (ld_res or N)
    a_in = strided_input(a, lda) if lda != K else a
    g_hi, g_lo = guarded((M, N), dtype, DEV, ld=ldc), guarded((M, N), dtype, DEV, ld=ldc)
    g_st = guarded((N // 64, M, 2), torch.float32, DEV) if want_stats else None
    if inplace:
        g_hi.view.copy_(hi)
        g_lo.view.copy_(lo)
        res = (g_hi.view, g_lo.view)
    else:
        res = (strided_input(hi, ld_res), strided_input(lo, ld_res))
    kw = dict(split_out=True, want_stats=want_stats)
    _, kernels = profiled(lambda: ops.linear_ex(a_in, w, b, res=res, inplace=inplace, lda=lda, ldc=ldc, ld_res=ld_res, out=g_hi.view,
                                                lo=g_lo.view, stats=g_st.view.view(N // 64, M, 2) if want_stats else None, **kw))
    res_intact = inplace or (torch.equal(res[0], hi) and torch.equal(res[1], lo))
    d = ops.linear_ex(a, w, b, res=(hi.clone(), lo.clone()), inplace=inplace, **kw)
    torch.cuda.synchronize()
    e = split_metrics(o, dtype, g_hi.view, g_lo.view, g_st.view if want_stats else None)
    same = torch.equal(g_hi.view, d["out"]) and torch.equal(g_lo.view, d["lo"])
    if want_stats:
        same = same and torch.equal(g_st.view.view(N // 64, M, 2), d["stats"])
    e.update(hi=g_hi, lo=g_lo, stats=g_st, kernels=kernels, bits_equal=bool(same), res_intact=bool(res_intact))
    return e


def attn_abi_case(B, N, dtype, mask_kind=None, seed=0):
    """bg_attn_fwd on a guarded output.  mask_kind: None | 'ragged' | 'one_empty' (ragged, and every key of sample 1 padded: its rows
    must be exactly 0; the fp64 reference is taken over the other samples)."""
    from guarded import guarded
    g = gen(seed)
    qkv = torch.randn(B * N, 2304, generator=g)
    qkv[:, :768] *= 0.125 * 2.0
    mask = None
    if mask_kind is not None:
        mask = torch.ones(B, N, dtype=torch.bool)
        for b in range(B):
            mask[b, : int(torch.randint(1, N + 1, (1,), generator=g))] = False
        if mask_kind == "one_empty":
            mask[1] = True
    qd = qkv.to(dtype)
    ref_mask = mask
    if mask_kind == "one_empty":                                  # (the reference yields NaN for that sample: give it one key, drop its rows)
        ref_mask = mask.clone()
        ref_mask[1, 0] = False
    want = _attn_ref(qd, ref_mask, B, N)
    out = guarded((B * N, 768), dtype, DEV)
    ops.attention(qd.to(DEV), mask.to(DEV) if mask is not None else None, B, N, out=out.view)
    torch.cuda.synchronize()
    got = out.view.float().cpu()
    keep = torch.ones(B * N, dtype=torch.bool)
    if mask_kind == "one_empty":
        keep[N:2 * N] = False
    e = _err(got[keep], want[keep])
    e.update(out=out, empty_rows_absmax=float(got[N:2 * N].abs().max()))     # (NaN, the sentinel included, compares unequal to 0)
    return e


def attn_varlen_abi_case(B, N, dtype, seed=0):
    """bg_attn_varlen_fwd on a guarded [B * N, 768] output with offsets that sum to fewer than B * N rows (one sample of N tokens, one
    of a single token).  Returns the error over the rows below offsets[B] and which rows were written at all."""
    from guarded import guarded
    g = gen(seed)
    nvalid = torch.randint(1, N + 1, (B,), generator=g)
    nvalid[0], nvalid[-1] = N, 1
    if B * N == int(nvalid.sum()):                                # (N = 1: nothing would be left over) a sample without rows
        nvalid[1] = 0
    offs = torch.zeros(B + 1, dtype=torch.int32)
    offs[1:] = torch.cumsum(nvalid, 0)
    total = int(offs[-1])
    qkv = torch.randn(B * N, 2304, generator=g)
    qkv[:, :768] *= 0.25
    qd = qkv.to(dtype)
    out = guarded((B * N, 768), dtype, DEV)
    offs_d = offs.to(DEV)
    ops.attention(qd.to(DEV), None, B, N, out=out.view, offsets=offs_d)
    torch.cuda.synchronize()
    worst = 0.0
    for b in range(B):
        lo, hi = int(offs[b]), int(offs[b + 1])
        if hi > lo:
            worst = max(worst, float((out.view[lo:hi].float().cpu().double() - _attn_ref(qd[lo:hi], None, 1, hi - lo)).abs().max()))
    written = out.written_mask()
    return {"max_abs": worst, "out": out, "total": total, "rows_below_all_written": bool(written[:total].all()),
            "rows_beyond_untouched": not bool(written[total:].any())}


def ln_silu_out_case(rows, n_out, dt, out=None):
    """bg_ln_silu_out_fwd vs the kernel's arithmetic in plain torch: fp64 LayerNorm of the 16-bit rows, SiLU, rounded to the operand
    dtype, exact product (operands as tests/test_gpu_round5.py draws them)."""
    g = torch.Generator().manual_seed(rows * 100 + n_out)
    t0 = (torch.randn(rows, 768, generator=g) * 1.7 + 0.3).to(dt)
    gamma, beta = 1 + 0.2 * torch.randn(768, generator=g), 0.1 * torch.randn(768, generator=g)
    w3 = (torch.randn(64, 768, generator=g) * 0.05).to(dt)
    b3 = torch.randn(64, generator=g)
    got = ops.ln_silu_out(t0.to(DEV), gamma.to(DEV), beta.to(DEV), w3.to(DEV), b3.to(DEV), n_out, out=out)
    h = torch.nn.functional.silu(torch.nn.functional.layer_norm(t0.double(), (768,), gamma.double(), beta.double(), 1e-5)).float().to(dt)
    want = (h.double() @ w3[:n_out].double().T + b3[:n_out].double()).float()
    return _err(got, want)
