"""`from src.dataset.locobot.locobot_singleview_dataloader import create_loaders, create_finetune_loaders,
create_transfer_loader` (reference file of the same path, :12-146)."""
from robot_aware_control_amd.data import create_finetune_loaders, create_transfer_loader  # noqa: F401
from robot_aware_control_amd.data import create_locobot_loaders as create_loaders  # noqa: F401
