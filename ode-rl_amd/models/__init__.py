from .ConvGRU import ConvGRU  # noqa: F401
from .gan import ConvNormAct, Discriminator, create_netD  # noqa: F401
from . import conv_odegru  # noqa: F401
from .conv_odegru import Encoder_z0_ODE_ConvGRU, DiffeqSolver  # noqa: F401
