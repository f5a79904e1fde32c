"""`from src.dataset.joint_pos_dataset import JointPosDataset, process_batch, get_batch` (reference src/dataset/joint_pos_dataset.py)."""
from robot_aware_control_amd.joint_pos_data import JointPosDataset, get_batch  # noqa: F401
from robot_aware_control_amd.robot_trainer import process_batch  # noqa: F401
