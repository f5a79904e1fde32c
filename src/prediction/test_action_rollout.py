"""`python -m src.prediction.test_action_rollout <trainer flags> --dynamics_model_ckpt CKPT [--step_size 0.02
--video_len 5 --nsample 3 --include_recorded True --out DIR]`

The reference's script of the same path: one batch of the experiment's test loader, its actions replaced by constant
pushes of +-step_size along x and y, the frozen checkpoint rolled out under each, one `<axis>_<mm>mm.gif` per sweep
with rows [ground truth | samples].  Here the sweeps and samples run as one batch and the sheets come from one launch
(`robot_aware_control_amd.action_rollout`); `--include_recorded True` adds the recorded actions as sweep "recorded" and
`response.json`, the mean absolute difference of every sweep's frames from that sweep's.

Flags are those of src/config/__init__.py.  What the reference hard-codes (`batch_size = 3`, `lstm_group_norm = True`,
the checkpoint path) is `--batch_size`, `--lstm_group_norm` and `--dynamics_model_ckpt` here; `--model copy` has no
weights and loads nothing.  A `finetune*` run of a model that takes masks or robot states rolls out on the robot model
the trainer builds (`--learned_robot_model True`); without one it is refused."""
import argparse
import os

import torch

from robot_aware_control_amd.config import create_env_probe, create_parser, str2bool


def tool_parser():
    """The flags of this tool alone, parsed in front of the trainer's flag table."""
    parser = argparse.ArgumentParser(add_help=False, allow_abbrev=False)  # (--video_len is no short form of anything)
    parser.add_argument("--step_size", type=float, default=0.02)  # metres per step (test_action_rollout.py:198)
    parser.add_argument("--video_len", type=int, default=5)
    parser.add_argument("--nsample", type=int, default=3)         # prior samples per video (--model svg)
    parser.add_argument("--include_recorded", type=str2bool, default=True)
    parser.add_argument("--out", type=str, default=".")           # the reference writes into the working directory
    return parser


def parse_args(argv=None):
    """(config, tool flags): the tool's parser first, the rest through the trainer's parser; an unknown flag aborts as
    in `config.argparser`."""
    tool, rest = tool_parser().parse_known_args(argv)
    config, unparsed = create_parser(create_env_probe(rest)).parse_known_args(rest)
    assert len(unparsed) == 0, unparsed
    return config, tool


def main(argv=None):
    from robot_aware_control_amd.action_rollout import probe
    from robot_aware_control_amd.data import experiment_loaders, get_batch
    from robot_aware_control_amd.trainer import PredictionTrainer
    config, tool = parse_args(argv)
    trainer = PredictionTrainer(config)  # the model, and the robot model such a run trains with
    if config.model != "copy":
        if not config.dynamics_model_ckpt:
            raise ValueError(f"--model {config.model} needs --dynamics_model_ckpt")
        ckpt = torch.load(config.dynamics_model_ckpt, map_location=config.device)
        trainer.model.load_state_dict(ckpt["model"])
    trainer.model.eval()
    _, test_loader, _ = experiment_loaders(config, transfer=False)
    data = next(get_batch(test_loader, config.device, prefetch=False))  # one batch: nothing to prefetch
    result = probe(trainer.model, config, data, step_size=tool.step_size, video_len=tool.video_len, nsample=tool.nsample,
                   include_recorded=tool.include_recorded, robot_model=trainer.robot_model)
    for path in result.write(tool.out):
        print(path)
    summary = result.summary()
    if summary is not None:
        for name, row in summary["sweeps"].items():
            print(f"{name}: mean |frame - recorded| {row['mean']:.6f}  per step " +
                  " ".join(f"{v:.6f}" for v in row["per_step"]))
    return result


if __name__ == "__main__":
    main()
