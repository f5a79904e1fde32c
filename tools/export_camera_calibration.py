"""Write the camera matrices the end-effector heatmaps need (`--model_use_heatmap`) to an .npz for
`--camera_calibration FILE`, where a reference checkout is present: its src/utils/camera_calibration.py holds the
measured extrinsics and intrinsics of the authors' rigs, which this repository does not carry.

    PYTHONPATH=<repo>:<reference> python tools/export_camera_calibration.py cameras.npz
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from robot_aware_control_amd.heatmaps import CameraTable  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    args = ap.parse_args()
    table = CameraTable.from_reference()
    table.save(args.out)
    print(f"wrote {args.out}: {len(table.world_to_camera)} viewpoints, {len(table.intrinsics)} cameras")


if __name__ == "__main__":
    main()
