"""`from src.dataset.locobot.locobot_table_dataloaders import create_loaders` (reference file of the same path,
:95-144)."""
from robot_aware_control_amd.data import create_locobot_table_loaders as create_loaders  # noqa: F401
