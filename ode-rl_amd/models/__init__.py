from .ConvGRU import ConvGRU  # noqa: F401
