"""`python -m src.prediction.measure_obj_movement --data_root R [trainer flags] [--views baxter/left_c0,widowx/widowx1_c0]
[--threshold X] [--overwrite True]`

The reference's script of the same path: writes `obj_movement.pkl` (and `obj_movement_scores.json`) into each viewpoint
folder, the table `--load_movement_info True` and `create_movement_loader` read.  Flags are those of
src/config/__init__.py; where the user gives none, `video_length`, `n_past`, `n_future`, `image_width` and `action_dim`
take the values the reference's `__main__` sets (measure_obj_movement.py:165-175).  Without `--views` it walks the
reference's robot -> viewpoints table and skips the folders the data root does not have."""
import argparse
import os

from robot_aware_control_amd.config import create_env_probe, create_parser, str2bool, str2list
from robot_aware_control_amd.movement import MOVEMENT_THRESHOLDS, ROBOT_VIEWPOINTS, measure_obj_movement  # noqa: F401

CLI_DEFAULTS = dict(video_length=31, n_past=1, n_future=30, image_width=64, action_dim=5)


def tool_parser():
    """The flags of this tool alone, parsed in front of the trainer's flag table."""
    parser = argparse.ArgumentParser(add_help=False)
    parser.add_argument("--views", type=str2list, default=None)   # robot/viewpoint_folder[,robot/viewpoint_folder...]
    parser.add_argument("--threshold", type=float, default=None)  # instead of MOVEMENT_THRESHOLDS, for every view
    parser.add_argument("--overwrite", type=str2bool, default=False)
    return parser


def parse_views(views):
    """["baxter/left_c0", ...] -> [("baxter", "left_c0"), ...]; None: the reference's table, in its order."""
    if not views:
        return [(robot, vp) for robot, vps in ROBOT_VIEWPOINTS.items() for vp in vps]
    pairs = []
    for v in views:
        robot, sep, vp = v.partition("/")
        if not (robot and sep and vp):
            raise ValueError(f"--views takes robot/viewpoint_folder pairs, got {v!r}")
        pairs.append((robot, vp))
    return pairs


def parse_args(argv=None):
    """(config, tool flags): the tool's parser first, the rest through the trainer's parser with this tool's defaults;
    an unknown flag aborts as in `config.argparser`."""
    tool, rest = tool_parser().parse_known_args(argv)
    parser = create_parser(create_env_probe(rest))
    parser.set_defaults(**CLI_DEFAULTS)
    config, unparsed = parser.parse_known_args(rest)
    assert len(unparsed) == 0, unparsed
    return config, tool


def main(argv=None):
    config, tool = parse_args(argv)
    for robot, vp in parse_views(tool.views):
        folder = os.path.join(config.data_root, f"{robot}_views", vp)
        if not tool.views and not os.path.isdir(folder):
            print(f"skipping {robot}/{vp}: {folder} does not exist")
            continue
        print(f"scoring {robot}/{vp}")
        measure_obj_movement(robot, vp, config, threshold=tool.threshold, overwrite=tool.overwrite)


if __name__ == "__main__":
    main()
