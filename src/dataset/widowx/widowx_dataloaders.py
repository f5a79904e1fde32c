"""`from src.dataset.widowx.widowx_dataloaders import create_finetune_loaders` (reference file of the same path,
:10-63)."""
from robot_aware_control_amd.data import create_widowx_finetune_loaders as create_finetune_loaders  # noqa: F401
