"""`from src.dataset.widowx.widowx_joint_pos_dataloaders import create_loaders` (reference file of the same path)."""
from robot_aware_control_amd.joint_pos_data import create_loaders  # noqa: F401
