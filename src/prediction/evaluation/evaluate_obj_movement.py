"""`python -m src.prediction.evaluation.evaluate_obj_movement --dynamics_model_ckpt CKPT --data_root R [trainer flags]`

The reference's script of the same path: a checkpoint's PSNR / SSIM over the high-movement videos
(`create_movement_loader`, the files `obj_movement.pkl` flags).  `--model copy` has no weights: nothing is loaded."""
from robot_aware_control_amd.config import argparser
from robot_aware_control_amd.data import create_movement_loader
from robot_aware_control_amd.trainer import PredictionTrainer
from src.prediction.multirobot_trainer import make_log_folder

KEYS = ("test/autoreg_psnr", "test/autoreg_ssim")


def compute_metrics(cf):
    """evaluate_obj_movement.py:13-21; returns the two numbers it prints."""
    trainer = PredictionTrainer(cf)
    if cf.model != "copy":
        trainer._step = trainer._load_checkpoint(cf.dynamics_model_ckpt)
    trainer.model.eval()
    info = trainer._compute_epoch_metrics(create_movement_loader(cf), "test")
    print("PSNR:", info[KEYS[0]])
    print("SSIM:", info[KEYS[1]])
    return {k: info[k] for k in KEYS}


def main(argv=None):
    config, _ = argparser(argv)
    config.log_dir = "ckpt_eval"
    make_log_folder(config)
    return compute_metrics(config)


if __name__ == "__main__":
    main()
