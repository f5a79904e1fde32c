"""`from src.dataset.baxter.baxter_joint_pos_dataloaders import create_finetune_loaders` (reference file of the same path)."""
from robot_aware_control_amd.joint_pos_data import create_finetune_loaders  # noqa: F401
