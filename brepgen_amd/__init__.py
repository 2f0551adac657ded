"""brepgen_amd -- MI355X-native (gfx950) implementation of BrepGen's latent-diffusion denoising hot path.

Drop-in for the reference's call surface on that path only:
    SurfPosNet / SurfZNet / EdgePosNet / EdgeZNet    (network.py)   -> bg_denoiser_fwd
    DDPMScheduler / PNDMScheduler                    (schedulers.py) -> bg_cfg_ddpm_step / bg_pndm_step
    randn_tensor                                     (utils.py)
    AutoencoderKLFastDecode / AutoencoderKL1DFastDecode (vae.py)    -> bg_im2col + GEMM, bg_small_attn, ...
    AutoencoderKL / AutoencoderKL1D / DiagonalGaussianDistribution (vae.py) -> the same programs + bg_vae_posterior
    compute_cov_mmd / jsd_between_point_cloud_sets   (metrics.py)   -> bg_chamfer_pairwise / bg_occupancy_counts
    sample_surface / sample_meshes                   (sample_points.py) -> bg_mesh_sample
    CADStore / augment_points (dataset.py: load_data, the six datasets) (dataset.py) -> bg_cad_filter / bg_batch_plan / bg_batch_gather
    dedup_cads / unique_items (data_process/deduplicate_*.py)       (deduplicate.py) -> bg_points_sha256 / bg_digest_group_keys / bg_first_occurrence
    optim.AdamW / optim.GradScaler / optim.clip_grad_norm_ (trainer.py's update) (optim.py) -> bg_mt_grad_stats / bg_mt_adamw_step / bg_optim_finish
    nn.MultiheadAttention in net.train() (attention core, dropout, backward) (attention.py) -> bg_attn_train_fwd / bg_attn_bwd
    nn.Linear of the encoder layers under autocast (forward, dX, dW + db) (linear.py) -> bg_weight_cast / bg_gemm_ex_fwd / bg_linear_wgrad
    nn.LayerNorm, ReLU, nn.Dropout and the residual adds of the encoder layers in net.train() (layer.py) -> bg_ln_train_fwd / bg_ln_bwd / bg_dropout_add_fwd / bg_relu_dropout_fwd
    the denoisers' embed MLPs / time_embed / fc_out and the masked-MSE loss in training (mlp.py, training.mse_loss) -> bg_thin_expand / bg_thin_contract / bg_thin_wgrad / bg_ln_silu_train_fwd / bg_ln_silu_bwd / bg_masked_mse_bwd
    the VAEs' ResnetBlock2D in training: GroupNorm + SiLU + 3x3 conv forward, dX, dW + db, GroupNorm backward (conv.py) -> bg_conv_wgrad / bg_conv_weight_pack / bg_gn_act_bwd + the VAE forward entries
    the VAEs' Downsample2D / Upsample2D convolutions in training, and whole down / up blocks (conv.py) -> bg_conv_wgrad_geom / bg_conv_down_dgrad / bg_conv_weight_pack_down / bg_pool2x2_sum
      (not built: the rest of the VAE backward -- conv_in / conv_out, mid-block attention, the 1-D blocks and resamplers, the
      posterior, a whole-VAE training step)
All compute goes through libbrepgen_hip.so (hand-written HIP kernels behind a C ABI, include/brepgen_hip.h).
"""
from . import optim  # noqa: F401
from .network import EdgePosNet, EdgeZNet, SurfPosNet, SurfZNet  # noqa: F401
from .schedulers import DDPMScheduler, PNDMScheduler  # noqa: F401
from .utils import randn_tensor  # noqa: F401
from .vae import (AutoencoderKL1DFastDecode, AutoencoderKL1DFastEncode, AutoencoderKLFastDecode,  # noqa: F401
                  AutoencoderKLFastEncode)

__all__ = ["SurfPosNet", "SurfZNet", "EdgePosNet", "EdgeZNet", "DDPMScheduler", "PNDMScheduler", "randn_tensor",
           "AutoencoderKLFastDecode", "AutoencoderKL1DFastDecode", "AutoencoderKLFastEncode",
           "AutoencoderKL1DFastEncode", "optim"]

# pc_metric.py's surface (metrics.py), resolved on first use: `python -m brepgen_amd.metrics` must find the module not yet imported
_METRICS = ("pairwise_chamfer", "compute_cov_mmd", "entropy_of_occupancy_grid", "jsd_between_point_cloud_sets",
            "jensen_shannon_divergence", "normalize_pc", "read_ply")
__all__ += list(_METRICS)
# sample_points.py's surface, likewise (`python -m brepgen_amd.sample_points`)
_SAMPLE_POINTS = ("sample_surface", "sample_meshes", "read_stl", "write_ply")
__all__ += list(_SAMPLE_POINTS)
# the full auto-encoders of the two VAE trainers (vae.py), next to the Fast classes above
_FULL_VAE = ("AutoencoderKL", "AutoencoderKL1D", "DiagonalGaussianDistribution")
__all__ += list(_FULL_VAE)
# dataset.py's surface (dataset.py): the training batches of the six trainers, assembled on the device
_DATASET = ("CADStore", "augment_points")
__all__ += list(_DATASET)
# data_process/deduplicate_cad.py and deduplicate_surfedge.py (deduplicate.py; `python -m brepgen_amd.deduplicate`)
_DEDUPLICATE = ("point_digests", "cad_keys", "first_occurrence", "dedup_cads", "unique_items")
__all__ += list(_DEDUPLICATE)
# the attention core for training: forward with dropout + backward on the device (attention.py)
_ATTENTION = ("self_attention", "MultiheadSelfAttention", "use_device_attention")
__all__ += list(_ATTENTION)
# the Linear layers of an encoder layer, forward and backward on the device (linear.py; the op itself is brepgen_amd.linear.linear:
# the package attribute `linear` is the submodule)
_LINEAR = ("DeviceLinear", "use_device_linear")
__all__ += list(_LINEAR)
# the rest of an encoder layer in training: LayerNorm forward / backward, dropout + residual add, ReLU + dropout (layer.py)
_LAYER = ("layer_norm", "dropout_add", "relu_dropout", "DeviceLayerNorm", "DeviceEncoderLayer", "use_device_layer")
__all__ += list(_LAYER)
# the denoisers' MLPs in training (mlp.py) and the differentiable loss / the one-call conversion of a denoiser (training.py)
_MLP = ("thin_linear_in", "thin_linear_out", "ln_silu", "DeviceMLP", "use_device_mlps")
_TRAINING = ("mse_loss", "use_device_training")
__all__ += list(_MLP + _TRAINING)
# the VAEs' ResnetBlock2D in training: GroupNorm + activation + convolution, forward and backward on the device (conv.py)
_CONV = ("gn_act_conv", "DeviceResnetBlock2D", "use_device_resnets", "conv_down", "conv_up", "DeviceDownsample2D", "DeviceUpsample2D",
         "DeviceBlock2D", "use_device_blocks")
__all__ += list(_CONV)


def __getattr__(name):
    if name in _METRICS:
        from . import metrics
        return getattr(metrics, name)
    if name in _SAMPLE_POINTS:
        from . import sample_points
        return getattr(sample_points, name)
    if name in _FULL_VAE:
        from . import vae
        return getattr(vae, name)
    if name in _DATASET:
        from . import dataset
        return getattr(dataset, name)
    if name in _DEDUPLICATE:
        from . import deduplicate
        return getattr(deduplicate, name)
    if name in _ATTENTION:
        from . import attention
        return getattr(attention, name)
    if name in _LINEAR:
        from . import linear
        return getattr(linear, name)
    if name in _LAYER:
        from . import layer
        return getattr(layer, name)
    if name in _MLP:
        from . import mlp
        return getattr(mlp, name)
    if name in _TRAINING:
        from . import training
        return getattr(training, name)
    if name in _CONV:
        from . import conv
        return getattr(conv, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
