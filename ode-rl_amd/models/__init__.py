from .ConvGRU import ConvGRU  # noqa: F401
from .gan import ConvNormAct, Discriminator, create_netD  # noqa: F401
