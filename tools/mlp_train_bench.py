#!/usr/bin/env python
"""The denoisers' MLPs and loss in training (csrc/mlp_train.hip, brepgen_amd/mlp.py, training.mse_loss) at the trainers' shapes.

Every case runs in a child process of its own under a time limit (a parent that never touches the device starts them one after another
and stops at the first that fails).
  * `kernels M` (M = 15 360 and 96 000 rows): each entry alone through the C ABI, windows of `--launches` launches between one pair of
    device events, `--rounds` windows per candidate, candidates alternating; reported are the median window's time per launch, the
    bytes the algorithm has to move (computed here from the shapes: every operand read once, every result written once, the fp64
    partials written and read back), and those bytes per second as a share of the 6.3 TB/s streaming rate of the CDNA guide.  For the
    thin products the fp32 FMAs (2 M 768 s FLOP) are reported too: at s = 48 they, not the bytes, are the floor.
  * `SurfZNet B S` / `EdgeZNet B S E` (512 x 30, 512 x 60 and 64 x 1500 tokens): forward + loss + backward of a 12-layer denoiser with
    the reference's module layout (built here: dropout 0.1, bf16 autocast) in the parent commit's best configuration
    (use_device_layer on the encoder, torch for the MLPs, loss_fn(pred[~mask], noise[~mask]): `parent`), the same a second time
    (`parent_again`: the spread) and after training.use_device_training with training.mse_loss (`device`), alternated, every call
    between its own device events.

    python tools/mlp_train_bench.py [--launches 100 --rounds 5 --warmup 2 --out profiles/r17/mlp_train_bench.json]
"""
import math
import os
import sys

from bench_common import phases, train_bench_main, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("kernels", 15360, 0, 0), ("kernels", 96000, 0, 0),
         ("SurfZNet", 512, 30, 0), ("SurfZNet", 512, 60, 0), ("SurfZNet", 64, 1500, 0),
         ("EdgeZNet", 512, 6, 5), ("EdgeZNet", 512, 6, 10), ("EdgeZNet", 64, 30, 50)]          # (what, B | M, S, E)
STREAM_RATE = 6.3e12
P, SEED, D = 0.1, 77, 768


def kernel_rows(torch, M, launches, rounds, warmup):
    from brepgen_amd import _lib
    lib = _lib.load()
    F32, BF = _lib.BG_F32, _lib.BG_BF16
    bf, s_ = torch.bfloat16, torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(M)
    rnd = lambda r, c, dt=torch.float32: torch.randn(r, c, generator=g, device="cuda").to(dt)       # noqa: E731
    p_ = lambda t: t.data_ptr()                                                                      # noqa: E731
    x18, u, dh = rnd(M, 18), rnd(M, D, bf), rnd(M, D, bf)
    y, h, dx = torch.empty(M, D, dtype=bf, device="cuda"), torch.empty(M, D, dtype=bf, device="cuda"), torch.empty(M, D, dtype=bf, device="cuda")
    gamma, beta = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    stats, dg, db = torch.empty(M, 2, device="cuda"), torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    nln = lib.bg_ln_silu_bwd_workspace_bytes(M)
    wsln = torch.empty(nln // 8, dtype=torch.float64, device="cuda")
    fns, need, flop = {}, {}, {}
    for s in (6, 12, 48):
        xs = x18[:, :s] if s <= 18 else rnd(M, s)
        ldx = xs.stride(0)
        w, w3, b, b3 = rnd(D, s), rnd(s, D), rnd(1, D).view(D), rnd(1, s).view(s)
        yo, gw, cs = torch.empty(M, s, device="cuda"), torch.empty(D, s, device="cuda"), torch.empty(D, device="cuda")
        nws = lib.bg_thin_wgrad_workspace_bytes(M, s)
        ws = torch.empty(nws // 8, dtype=torch.float64, device="cuda")
        fns[f"thin_expand s={s}"] = (lambda xs=xs, ldx=ldx, w=w, b=b, s=s:
                                     lib.bg_thin_expand(p_(xs), F32, ldx, p_(w), 0, p_(b), p_(y), BF, M, s, s_))
        fns[f"thin_contract n={s}"] = lambda w3=w3, b3=b3, yo=yo, s=s: lib.bg_thin_contract(p_(u), BF, p_(w3), p_(b3), p_(yo), M, s, s_)
        fns[f"thin_wgrad s={s}"] = (lambda xs=xs, ldx=ldx, gw=gw, cs=cs, ws=ws, nws=nws, s=s:
                                    lib.bg_thin_wgrad(p_(xs), F32, ldx, p_(u), BF, p_(gw), 1, p_(cs), 1, M, s, p_(ws), nws, s_))
        thin, wide = float(M) * s * 4, float(M) * D * 2
        need[f"thin_expand s={s}"] = thin + wide + D * s * 4
        need[f"thin_contract n={s}"] = thin + wide + D * s * 4
        need[f"thin_wgrad s={s}"] = thin + wide + 2.0 * nws + D * s * 4
        for k in ("thin_expand s=", "thin_contract n=", "thin_wgrad s="):
            flop[f"{k}{s}"] = 2.0 * M * D * s
    fns["ln_silu_train_fwd"] = lambda: lib.bg_ln_silu_train_fwd(p_(u), BF, p_(gamma), p_(beta), p_(h), BF, p_(stats), M, 1e-5, s_)
    fns["ln_silu_bwd"] = lambda: lib.bg_ln_silu_bwd(p_(dh), BF, p_(u), BF, p_(stats), p_(gamma), p_(beta), p_(dx), p_(dg), p_(db), M, p_(wsln), nln, s_)
    fns["ln_silu_bwd_dx_only"] = lambda: lib.bg_ln_silu_bwd(p_(dh), BF, p_(u), BF, p_(stats), p_(gamma), p_(beta), p_(dx), None, None, M, None, 0, s_)
    need["ln_silu_train_fwd"] = float(M) * D * 4 + 8.0 * M
    need["ln_silu_bwd"] = float(M) * D * 6 + 8.0 * M + 2.0 * nln
    need["ln_silu_bwd_dx_only"] = float(M) * D * 6 + 8.0 * M
    for ld in (18, 48):
        pred, target, dpred = rnd(M, ld), rnd(M, ld), torch.empty(M, ld, device="cuda")
        mask = (torch.rand(M, generator=g, device="cuda") < 0.2).to(torch.uint8)
        scratch, out3, gs = torch.empty(1024, dtype=torch.float64, device="cuda"), torch.empty(3, device="cuda"), torch.ones(1, device="cuda")
        _lib.check(lib.bg_masked_mse(p_(pred), p_(target), p_(mask), M, ld, 0, ld, p_(scratch), p_(out3), s_), "bg_masked_mse")
        fns[f"masked_mse_bwd ld={ld}"] = (lambda pred=pred, target=target, mask=mask, out3=out3, gs=gs, dpred=dpred, ld=ld:
                                          lib.bg_masked_mse_bwd(p_(pred), p_(target), p_(mask), M, ld, 0, ld, p_(out3), p_(gs), p_(dpred), s_))
        need[f"masked_mse_bwd ld={ld}"] = float(M) * ld * 12 + M
    for name, f in fns.items():
        _lib.check(f(), name)
    t = windows(torch, fns, launches, rounds, warmup)
    rows = []
    for k in fns:
        row = {"kernel": k, "M": M, "ms": round(t[k], 5), "bytes_needed": need[k], "tb_per_s": round(need[k] / (t[k] * 1e-3) / 1e12, 3),
               "share_of_stream_rate": round(need[k] / (t[k] * 1e-3) / STREAM_RATE, 3)}
        if k in flop:
            row["fp32_tflops"] = round(flop[k] / (t[k] * 1e-3) / 1e12, 2)
        rows.append(row)
    return rows


def build_denoiser(torch, kind):
    """A 12-layer denoiser with the reference's module layout and state-dict keys (network.py:1076-1099), written out here: tools/ does
    not import the checker."""
    import torch.nn as nn

    def seq(k, n):
        return nn.Sequential(nn.Linear(k, D), nn.LayerNorm(D), nn.SiLU(), nn.Linear(D, n))

    embeds = {"SurfZNet": {"z_embed": 48, "p_embed": 6},
              "EdgeZNet": {"surfz_embed": 48, "edgez_embed": 12, "surfp_embed": 6, "edgep_embed": 6, "vertp_fc": 6}}[kind]

    class Denoiser(nn.Module):
        def __init__(self):
            super().__init__()
            layer = nn.TransformerEncoderLayer(d_model=D, nhead=12, norm_first=True, dim_feedforward=1024, dropout=P)
            self.net = nn.TransformerEncoder(layer, 12, nn.LayerNorm(D), enable_nested_tensor=False)
            for name, k in embeds.items():
                setattr(self, name, seq(k, D))
            self.time_embed = seq(D, D)
            self.fc_out = seq(D, 48 if kind == "SurfZNet" else 18)

        def cond(self, t):
            f = torch.exp(-math.log(10000.0) * torch.arange(D // 2, dtype=torch.float32, device=t.device) / (D // 2))
            a = t[:, None].float() * f[None]
            return self.time_embed(torch.cat([torch.cos(a), torch.sin(a)], dim=-1)).unsqueeze(1)

        def encode(self, tok, key_pad):
            return self.fc_out(self.net(src=tok.permute(1, 0, 2), src_key_padding_mask=key_pad).transpose(0, 1))

        def forward(self, *args):
            if kind == "SurfZNet":
                z, t, pos, mask = args
                return self.encode(self.z_embed(z) + self.p_embed(pos) + self.cond(t), mask)
            ez, t, ep, pos, z, mask = args
            B, S, E, _ = ep.shape
            surf = (self.surfp_embed(pos) + self.surfz_embed(z)).unsqueeze(2).repeat(1, 1, E, 1)
            tok = self.edgep_embed(ep) + self.edgez_embed(ez[..., :12]) + self.vertp_fc(ez[..., 12:]) + surf
            tok = tok.reshape(B, S * E, D) + self.cond(t)
            return self.encode(tok, mask.reshape(B, S * E)).reshape(B, S, E, -1)

    return Denoiser()


def step_row(torch, kind, B, S, E, iters, rounds, warmup):
    import copy

    import torch.nn.functional as F

    import brepgen_amd as bga
    from brepgen_amd import training
    torch.manual_seed(S)
    base = build_denoiser(torch, kind).cuda().train()
    models = {}
    for name in ("parent", "parent_again"):
        models[name] = copy.deepcopy(base)
        bga.use_device_layer(models[name].net, seed=SEED)
    models["device"] = training.use_device_training(copy.deepcopy(base), seed=SEED)
    g = torch.Generator(device="cuda").manual_seed(B)
    rnd = lambda *shape: torch.randn(*shape, generator=g, device="cuda")                            # noqa: E731
    t = torch.randint(0, 1000, (B,), generator=g, device="cuda")
    if kind == "SurfZNet":
        mask = torch.zeros(B, S, dtype=torch.bool, device="cuda")
        mask[:, S - S // 5:] = True
        args, noise = (rnd(B, S, 48), t, rnd(B, S, 6), mask), rnd(B, S, 48)
    else:
        mask = torch.zeros(B, S, E, dtype=torch.bool, device="cuda")
        mask[:, :, E - E // 5:] = True
        args, noise = (rnd(B, S, E, 18), t, rnd(B, S, E, 6), rnd(B, S, 6), rnd(B, S, 48), mask), rnd(B, S, E, 18)
    ev = lambda: torch.cuda.Event(enable_timing=True)                                              # noqa: E731

    def run(model, device_loss):
        def call():
            model.zero_grad(set_to_none=True)
            a, c, d = ev(), ev(), ev()
            a.record()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                pred = model(*args)
                loss = training.mse_loss(pred, noise, mask) if device_loss else F.mse_loss(pred[~mask], noise[~mask])
            c.record()
            loss.backward()
            d.record()
            return a, c, d
        return call

    tm = phases(torch, {k: run(m, k == "device") for k, m in models.items()}, iters, rounds, warmup, 2)
    row = {"net": kind, "B": B, "S": S, "E": E, "tokens": B * S * max(E, 1)}
    for k, v in tm.items():
        row[k] = {"fwd_loss_ms": round(v[0], 3), "bwd_ms": round(v[1], 3), "total_ms": round(sum(v), 3)}
    row["spread_parent_vs_itself"] = round(abs(row["parent"]["total_ms"] - row["parent_again"]["total_ms"]) / row["parent"]["total_ms"], 4)
    row["device_over_parent"] = round(row["device"]["total_ms"] / row["parent"]["total_ms"], 4)
    return row


def child(what, B, S, E, args):
    import torch
    if what == "kernels":
        return kernel_rows(torch, B, args.launches, args.rounds, args.warmup)
    return [step_row(torch, what, B, S, E, 3, args.rounds, args.warmup)]


def main():
    return train_bench_main(__file__, os.path.join(ROOT, "profiles", "r17", "mlp_train_bench.json"), CASES, ("what", "B_or_M", "S", "E"), child,
                            lambda a: {"stream_rate_bytes_per_s": STREAM_RATE, "launches_per_window": a.launches, "rounds": a.rounds,
                                       "dropout_p": P, "autocast": "bfloat16"}, launches=100)


if __name__ == "__main__":
    sys.exit(main())
