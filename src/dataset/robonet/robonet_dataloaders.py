"""`from src.dataset.robonet.robonet_dataloaders import create_loaders, create_movement_loader` (reference
robonet_dataloaders.py:21-80, 295-327)."""
from robot_aware_control_amd.data import create_loaders, create_movement_loader  # noqa: F401
