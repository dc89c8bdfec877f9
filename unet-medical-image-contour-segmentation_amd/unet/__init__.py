from .unet_model import UNet, UNet_S, UNet_SA, UNet_T, UNetDepth  # noqa: F401
from .unet_parts import AttentionUp, DoubleConv, Down, OutConv, SpatialAttention, Up  # noqa: F401
