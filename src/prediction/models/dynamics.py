"""`from src.prediction.models.dynamics import SVGConvModel, DeterministicConvModel, CopyModel`
(reference dynamics.py:457-644, :363-454, :341-360), and the learned robot model's `JointPosPredictor`, `GripperStatePredictor`
(:269-338)."""
from robot_aware_control_amd.model import CopyModel, DeterministicConvModel, SVGConvModel  # noqa: F401
from robot_aware_control_amd.robot_model import GripperStatePredictor, JointPosPredictor  # noqa: F401
