"""MI355X-native Neural-ODE hot path of jithendaraa/ODE-RL.

Public surface = the reference's: `odeint`, `DiffEqSolver`, `ODEFunc`, `create_convnet`.
"""
from . import _lib  # noqa: F401
from .odeint import odeint, last_stats, step_size_grid  # noqa: F401
from .autograd import odeint_adjoint, last_adjoint_stats, sample_z0, last_z0_noise, mse_kl_loss, vidode_l1_loss  # noqa: F401
from .autograd import instnorm_lrelu, gan_sequences, lsgan_loss  # noqa: F401
from .hip_ops import set_compute_dtype, set_bf16_tanh, current_compute_dtype, set_async_dopri5, collect_pending_solves, set_adjoint_grids, set_reverse_time_grads  # noqa: F401
from .helpers.utils import create_convnet  # noqa: F401
from .modules.DiffEqSolver import DiffEqSolver, ODEFunc  # noqa: F401
from .modules.ConvGRUCell import ConvGRUCell  # noqa: F401
from .modules.ODEConvGRUCell import ODEConvGRUCell  # noqa: F401
from .metrics import frame_metrics, FrameMetrics, png_metrics, PngMetrics, PngEvaluation  # noqa: F401
from .optim import FusedAdam, FusedAdamax, decay_learning_rate  # noqa: F401
from .models.gan import ConvNormAct, Discriminator, create_netD  # noqa: F401
from .train import train_batch_gan  # noqa: F401
from . import vidode_data  # noqa: F401
from .vidode_data import ClipStore, VidODEBatches  # noqa: F401
# upstream Vid-ODE's own model; its ConvGRUCell, ODEFunc, create_convnet and VidODE share names with the classes above and live in the module
from .models import conv_odegru  # noqa: F401
from .models.conv_odegru import Encoder_z0_ODE_ConvGRU, DiffeqSolver  # noqa: F401

__all__ = ["odeint", "odeint_adjoint", "DiffEqSolver", "ODEFunc", "create_convnet", "ConvGRUCell", "ODEConvGRUCell", "frame_metrics",
           "FrameMetrics", "sample_z0", "last_z0_noise", "mse_kl_loss", "vidode_l1_loss", "step_size_grid", "set_adjoint_grids", "set_reverse_time_grads", "FusedAdam", "FusedAdamax",
           "decay_learning_rate", "instnorm_lrelu", "gan_sequences", "lsgan_loss", "ConvNormAct", "Discriminator", "create_netD",
           "train_batch_gan", "conv_odegru", "Encoder_z0_ODE_ConvGRU", "DiffeqSolver", "vidode_data", "ClipStore", "VidODEBatches",
           "png_metrics", "PngMetrics", "PngEvaluation"]
