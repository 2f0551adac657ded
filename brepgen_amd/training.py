"""Forward half of the reference's LDM trainers on the device: VAE encode -> latent tokens
-> ``add_noise`` -> eps-net -> masked MSE, i.e. everything ``trainer.py`` does between loading a batch and calling
``backward()``, and all of its ``test_val`` loops (trainer.py:374-408, 557-602, 752-797, 975-1030).  These functions run under
``no_grad`` on the package's inference modules: they let the same kernels compute the training / validation *losses* of a
checkpoint (the differentiable loss is ``mse_loss``, below).  ``vae_loss`` / ``vae_validation`` are the same for the two VAE trainers
(SurfVAETrainer / EdgeVAETrainer, trainer.py:62-129, 190-259): encode -> sample the posterior -> decode -> MSE + 1e-6 KL.

Every function takes and returns device tensors and enqueues on the current stream; nothing synchronises.
"""
import torch

from . import _lib
from ._lib import check, ptr, stream

VAL_STEPS = (10, 50, 100, 200, 500)          # timesteps the reference validates at (trainer.py:394, 587, 781, 1008)


def _row_mask(mask, pred):
    """mask broadcast over pred's rows (EdgePosNet: the [B, S] face mask over [B, S, E, 6] edges), as contiguous uint8, or None.
    Whether it covers the rows is the caller's check."""
    if mask is None:
        return None
    if mask.dim() < pred.dim() - 1:
        mask = mask.unsqueeze(-1).expand(pred.shape[:-1])
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)


def _launch_mse(pred, target, mask, c0, c1):
    """bg_masked_mse on fp32 pred / target [..., C] and a uint8 row mask (or None): (p, t, out) -- the contiguous operands and
    out = (mean, row_mean_sum, rows) on the device"""
    C = pred.shape[-1]
    p, t = pred.contiguous(), target.contiguous()
    scratch = torch.empty(1024, device=p.device, dtype=torch.float64)
    out = torch.empty(3, device=p.device, dtype=torch.float32)
    check(_lib.load().bg_masked_mse(ptr(p), ptr(t), ptr(mask), p.numel() // C, C, c0, c1 - c0, ptr(scratch), ptr(out), stream()),
          "bg_masked_mse")
    return p, t, out


def masked_mse(pred, target, mask=None, cols=None):
    """``nn.MSELoss()(pred[~mask], target[~mask])`` and the ``test_val`` reduction, from one deterministic kernel pair.

    pred / target: fp32 [..., C]; mask: bool [...] (True = padded) or None; cols: (start, stop) column slice or None
    (EdgeZTrainer also reports the latent 0:12 and vertex 12:18 parts, trainer.py:951-952).
    Returns {"mean": scalar tensor, "row_mean_sum": sum over valid rows of the per-row mean, "rows": valid rows}."""
    if not pred.is_cuda:
        raise _lib.BrepgenHipError(f"brepgen_amd runs on the MI355X only (tensor on {pred.device}); no CPU fallback")
    assert pred.shape == target.shape and pred.dtype == torch.float32 and target.dtype == torch.float32
    assert mask is None or mask.shape == pred.shape[:-1]
    c0, c1 = cols if cols is not None else (0, pred.shape[-1])
    _, _, out = _launch_mse(pred, target, _row_mask(mask, pred), c0, c1)
    return {"mean": out[0], "row_mean_sum": out[1], "rows": out[2]}


class _MseLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mask, cols):
        p, t, out = _launch_mse(pred, target, mask, *cols)
        ctx.save_for_backward(p, t, mask, out)
        ctx.dims = (p.numel() // pred.shape[-1], pred.shape[-1], cols)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        p, t, mask, out = ctx.saved_tensors
        rows, C, cols = ctx.dims
        g = g.detach().to(torch.float32).contiguous()
        dpred = torch.empty_like(p)
        check(_lib.load().bg_masked_mse_bwd(ptr(p), ptr(t), ptr(mask), rows, C, cols[0], cols[1] - cols[0], ptr(out), ptr(g), ptr(dpred), stream()),
              "bg_masked_mse_bwd")
        return dpred, None, None, None


def mse_loss(pred, target, mask=None, cols=None):
    """``nn.MSELoss()(pred[~mask], target[~mask])`` as a differentiable scalar (trainer.py:354, 537, 732, 950): forward ``bg_masked_mse``,
    backward ``bg_masked_mse_bwd`` -- dpred = 2 (pred - target) g / (valid rows * columns) on the compared elements and exactly 0
    elsewhere, the count of valid rows read on the device, so neither direction synchronises (``pred[~mask]`` does).

    pred [..., C] fp32, or fp16 / bf16 as autocast's fc_out hands it over (cast to fp32 first, as autocast's mse_loss does); target
    fp32 [..., C], must not require a gradient; mask bool [...] (True = padded), broadcast over trailing row dimensions as in
    ``ldm_loss``; cols (start, stop) or None.  With no valid row the loss and its gradient are 0."""
    if target.requires_grad:
        raise ValueError("mse_loss: target requires a gradient; only pred is differentiated")
    if pred.shape != target.shape or pred.dim() < 1 or not pred.is_floating_point():
        raise ValueError(f"mse_loss: pred {tuple(pred.shape)} {pred.dtype} and target {tuple(target.shape)} must be floating tensors of one shape")
    C = pred.shape[-1]
    c0, c1 = (0, C) if cols is None else (int(cols[0]), int(cols[1]))
    if not 0 <= c0 < c1 <= C:
        raise ValueError(f"mse_loss: cols = {cols} outside the {C} columns")
    if not pred.is_cuda or not target.is_cuda:
        raise _lib.BrepgenHipError(f"mse_loss runs on the MI355X only (tensors on {pred.device} / {target.device}); no CPU fallback")
    mask = _row_mask(mask, pred)
    if mask is not None and mask.shape != pred.shape[:-1]:
        raise ValueError(f"mse_loss: mask {tuple(mask.shape)} does not cover the rows of pred {tuple(pred.shape)}")
    with torch.autocast(device_type="cuda", enabled=False):
        return _MseLoss.apply(pred.float(), target.detach().float(), mask, (c0, c1))


def use_device_training(model, seed=None):
    """Convert a reference-keyed denoiser (``net``: the nn.TransformerEncoder; the embed MLPs, ``time_embed`` and ``fc_out`` as direct
    children) for training on this library: ``layer.use_device_layer(model.net, seed)`` and ``mlp.use_device_mlps(model)``.
    Parameter objects and state_dict keys are unchanged.  Launches nothing.  Returns the model."""
    from .layer import use_device_layer
    from .mlp import use_device_mlps
    if not hasattr(model, "net"):
        raise ValueError("use_device_training: a denoiser with its nn.TransformerEncoder as .net is required")
    use_device_layer(model.net, seed)
    return use_device_mlps(model)


def augment(ddpm, conditions, generator=None, max_t=15):
    """Conditioning augmentation of the Z / edge trainers (trainer.py:507-514, 935-941): a little forward diffusion
    (t ~ U{0..14}) on every conditioning tensor.  Draws on the CPU generator like utils.randn_tensor."""
    out = []
    for x in conditions:
        t = torch.randint(0, max_t, (x.shape[0],), generator=generator)
        noise = torch.randn(x.shape, generator=generator).to(x.device)
        out.append(ddpm.add_noise(x, noise, t))
    return out


@torch.no_grad()
def ldm_loss(net, ddpm, x0, timesteps, noise, conditions=(), mask=None, class_label=None, is_train=False, cols=None):
    """One loss evaluation of any of the four LDM trainers: diffuse x0 to per-sample ``timesteps`` with ``noise``
    (trainer.py:346-348), predict it with ``net(x_t, timesteps, *conditions[, mask], class_label, is_train)``
    (trainer.py:351, 534, 729, 947) and compare on the un-padded rows (trainer.py:354, 537, 732, 950)."""
    x_t = ddpm.add_noise(x0, noise, timesteps)
    args = [x_t, timesteps, *conditions] + ([mask] if mask is not None else []) + [class_label]
    pred = net(*args, is_train) if is_train else net(*args)
    return masked_mse(pred, noise.to(pred.device), _row_mask(mask, pred), cols)


@torch.no_grad()
def validation_losses(net, ddpm, x0, conditions=(), mask=None, class_label=None, generator=None, steps=VAL_STEPS):
    """The body of ``test_val`` for one batch: loss at t = step-1 for step in (10, 50, 100, 200, 500) with fresh noise
    each (trainer.py:394-401, 587-597).  Returns a list of dicts as from masked_mse, one per step."""
    B = x0.shape[0]
    out = []
    for step in steps:
        t = torch.full((B,), step - 1, dtype=torch.int64, device=x0.device)       # randint(step-1, step) has one value
        noise = torch.randn(x0.shape, generator=generator).to(x0.device)
        out.append(ldm_loss(net, ddpm, x0, t, noise, conditions, mask, class_label))
    return out


@torch.no_grad()
def surface_tokens(surf_vae_encoder, surfPnt, z_scaled=1.0):
    """trainer.py:519-526: point grids [B,S,32,32,3] -> VAE posterior mode -> rescaled latent tokens [B,S,48]."""
    return surf_vae_encoder.encode_tokens(surfPnt) * z_scaled


@torch.no_grad()
def edge_tokens(edge_vae_encoder, edgePnt, vertPos, z_scaled=1.0):
    """trainer.py:924-933: polylines [B,S,E,32,3] -> latent tokens [B,S,E,12], concatenated with the 6 vertex
    coordinates -> the 18-channel joint data EdgeZNet denoises."""
    return torch.cat([edge_vae_encoder.encode_tokens(edgePnt) * z_scaled, vertPos], -1)


def _vae_pass(vae, x, generator, noise):
    """encode -> posterior.sample() -> decode, channels-last throughout: (x_cl, posterior, dec_cl, restore)."""
    x_cl, restore = vae._points_cl(x)
    posterior = vae._encode_cl(x_cl)
    dec_cl = vae._decode_cl(posterior._sample_cl(generator, noise))
    return x_cl, posterior, dec_cl, restore


@torch.no_grad()
def vae_loss(vae, x, generator=None, noise=None, kl_weight=1e-6):
    """The loss of one SurfVAETrainer / EdgeVAETrainer step (trainer.py:79-86, 206-216) for a full ``AutoencoderKL`` /
    ``AutoencoderKL1D``: mse = nn.MSELoss()(dec, x), kl = posterior.kl().mean(), total = mse + kl_weight * kl.

    x: points in the datasets' layout [..., 32, 32, 3] / [..., 32, 3] or the trainers' permuted [n, 3, 32, 32] / [n, 3, 32]; ``dec``
    comes back in the same layout.  noise [n, 3, 4, 4] / [n, 3, 4]: the posterior's eps (parity with a reference run); otherwise the
    kernel draws it under ``sampling.noise_key(generator)`` -- deterministic: the same generator state gives the same loss."""
    x_cl, posterior, dec_cl, restore = _vae_pass(vae, x, generator, noise)
    n = x_cl.shape[0]
    mse = masked_mse(dec_cl.reshape(n, -1), x_cl.reshape(n, -1))["mean"]          # rows = samples, no mask
    kl_per_sample = posterior.kl()
    kl = kl_per_sample.mean()
    return {"mse": mse, "kl": kl, "total": mse + kl_weight * kl, "dec": restore(dec_cl), "kl_per_sample": kl_per_sample}


@torch.no_grad()
def vae_validation(vae, x, generator=None, noise=None):
    """The body of the VAE trainers' ``test_val`` for one batch (trainer.py:118-124, 248-254): the posterior is SAMPLED, then
    mse_sum = mse(reduction='none')(dec, x).mean(all but batch).sum() and count = len(x); the epoch's figure is sum / sum."""
    x_cl, _, dec_cl, _ = _vae_pass(vae, x, generator, noise)
    n = x_cl.shape[0]
    return {"mse_sum": masked_mse(dec_cl.reshape(n, -1), x_cl.reshape(n, -1))["row_mean_sum"], "count": n}
