"""`from src.prediction.joint_pos_trainer import RobotPredictionTrainer` (reference src/prediction/joint_pos_trainer.py):
training of the learned robot model's two predictors.  The reference's joint-position dataloaders are not built, so there
is no command line here: build the trainer and hand `train` a batch generator and a test loader."""
from robot_aware_control_amd.robot_trainer import RobotPredictionTrainer, process_batch  # noqa: F401
