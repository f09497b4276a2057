from .fused_adamw import FusedAdamW  # noqa: F401
from .norms import total_norms  # noqa: F401
