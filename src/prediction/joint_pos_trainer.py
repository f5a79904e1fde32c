"""`python -um src.prediction.joint_pos_trainer --jobname ... --experiment finetune_widowx --data_root ...`

The reference's entry point of the same path: trains the learned robot model's two predictors on the joint-position
data under the data root (`finetune_widowx`: <data_root>/widowx_views/*/, `finetune_baxter`:
<data_root>/baxter_views/left_c0) and writes the checkpoints `--robot_model_ckpt` takes.  Flags are those of
src/config/__init__.py; `--plot True` adds the mask GIFs and the mask IoU."""
import numpy as np
import torch

from robot_aware_control_amd.config import argparser
from robot_aware_control_amd.robot_trainer import RobotPredictionTrainer, process_batch  # noqa: F401
from src.prediction.multirobot_trainer import make_log_folder


def main(argv=None):
    config, _ = argparser(argv)
    torch.manual_seed(config.seed)
    np.random.seed(config.seed)
    make_log_folder(config)
    trainer = RobotPredictionTrainer(config)
    trainer.train()
    return trainer


if __name__ == "__main__":
    main()
