"""The file tree, the flags and the cases of the experiment-split tests: shared by tests/test_experiment_loaders_host.py
and tools/gen_golden_splits.py (which records the reference's own splits of this tree in
tests/golden/experiment_splits.json)."""
import argparse
import os
import pickle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "experiment_splits.json")
SAWYER_VIEWS = ["sudri0_c0", "sudri0_c1", "sudri0_c2", "sudri2_c0", "sudri2_c1", "sudri2_c2", "vestri_table2_c0",
                "vestri_table2_c1", "vestri_table2_c2"]
# (folder, files): enough locobot files for the fixed 200 + 3000 and 1000 + 10000 splits to leave a train part
TREE = ([(f"sawyer_views/{v}", 14 if v == "sudri2_c1" else 6) for v in SAWYER_VIEWS]
        + [("widowx_views/widowx1_c0", 15), ("baxter_views/left_c0", 7)]
        + [(f"locobot_views/c{i}", 55 + i) for i in range(4)] + [("locobot_table_views/c0", 1012)])
SCORED = ("sawyer_views/sudri2_c1", "widowx_views/widowx1_c0")  # the folders the world-error pickle covers
EXPERIMENTS = ("train_robonet", "train_sawyer_multiview", "finetune_sawyer_view", "finetune_widowx",
               "train_locobot_singleview", "finetune_locobot", "train_locobot_table")
SEEDS = (0, 3)
WORLD_ERROR = "world_error.pkl"


def moves(i: int) -> bool:
    """Whether file i of a scored folder counts as high-movement."""
    return i % 4 != 1


def write_tree(root, movement_tables=False):
    """Empty traj_###.hdf5 files (the loaders only list them) and the world-error pickle over the scored folders, in the
    reference's layout {path: [{"high_error": bool}, ...]}.  `movement_tables`: also each scored folder's
    obj_movement.pkl with the same flags.  Returns the pickle's path."""
    info = {}
    for folder, n in TREE:
        d = os.path.join(root, folder)
        os.makedirs(d, exist_ok=True)
        table = {}
        for i in range(n):
            path = os.path.join(d, f"traj_{i:03d}.hdf5")
            open(path, "wb").close()
            if folder in SCORED:
                info[path] = [{"high_error": False}, {"high_error": moves(i)}]
                table[path] = moves(i)
        if movement_tables and folder in SCORED:
            with open(os.path.join(d, "obj_movement.pkl"), "wb") as f:
                pickle.dump(table, f)
    path = os.path.join(root, WORLD_ERROR)
    with open(path, "wb") as f:
        pickle.dump(info, f)
    return path


def config(root, experiment, seed, **kw):
    d = dict(data_root=root, experiment=experiment, seed=seed, world_error_dict=os.path.join(root, WORLD_ERROR),
             finetune_num_test=3, finetune_num_train=5, train_val_split=0.8, img_augmentation=False, data_threads=0,
             batch_size=4, test_batch_size=3, load_movement_info=False, video_length=5, n_past=1, n_future=2,
             action_dim=4, robot_dim=5, robot_joint_dim=7, impute_autograsp_action=False, image_width=64,
             image_height=48, preload_ram=False, preprocess_action="raw", model_use_heatmap=False, device_images=False,
             device_resident=False)
    d.update(kw)
    return argparse.Namespace(**d)


def case_key(experiment, seed):
    return f"{experiment}/seed{seed}"
