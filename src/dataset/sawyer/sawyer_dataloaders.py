"""`from src.dataset.sawyer.sawyer_dataloaders import create_loaders, create_transfer_loader,
create_finetune_loaders` (reference file of the same path, :18-190)."""
from robot_aware_control_amd.data import SAWYER_MULTIVIEW_TRAIN_DIRS as SAWYER_TRAIN_DIRS  # noqa: F401
from robot_aware_control_amd.data import create_sawyer_finetune_loaders as create_finetune_loaders  # noqa: F401
from robot_aware_control_amd.data import create_sawyer_loaders as create_loaders  # noqa: F401
from robot_aware_control_amd.data import create_sawyer_transfer_loader as create_transfer_loader  # noqa: F401
