"""TEST INFRASTRUCTURE ONLY -- the reference's train / test / transfer splits of every `--experiment` its trainer knows.

Runs only where the reference checkout is present: it loads oracle/gen_golden.py for its recipe (absent third-party
modules stubbed, the reference first on sys.path so that the name `src` is the reference's; scikit-learn is the real
one: `train_test_split` is part of what is recorded), imports the REFERENCE's own loader functions, replaces the
dataset and the DataLoader they build by recorders, and runs them over the tree of empty files of
tests/experiment_split_refs.py for every experiment and seed.  It records relative paths, labels, batch sizes and
shuffle flags only, to tests/golden/experiment_splits.json.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_splits.py
"""
import importlib
import importlib.util
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


gg = _load("gen_golden", os.path.join(REPO, "oracle", "gen_golden.py"))  # stubs + sys.path: the reference imports now
refs = _load("experiment_split_refs", os.path.join(REPO, "tests", "experiment_split_refs.py"))
gg.MISSING.discard("sklearn")
for name in [m for m in sys.modules if m.split(".")[0] == "sklearn"]:
    del sys.modules[name]  # (a stub an earlier import left behind)

# --experiment -> (module, loaders, transfer loader or None): the choice of the reference's trainer.py:899-947
CHOICE = {
    "train_robonet": ("src.dataset.robonet.robonet_dataloaders", "create_loaders",
                      ("src.dataset.locobot.locobot_singleview_dataloader", "create_transfer_loader")),
    "train_sawyer_multiview": ("src.dataset.sawyer.sawyer_dataloaders", "create_loaders",
                               ("src.dataset.sawyer.sawyer_dataloaders", "create_transfer_loader")),
    "finetune_sawyer_view": ("src.dataset.sawyer.sawyer_dataloaders", "create_finetune_loaders", None),
    "finetune_widowx": ("src.dataset.widowx.widowx_dataloaders", "create_finetune_loaders", None),
    "train_locobot_singleview": ("src.dataset.locobot.locobot_singleview_dataloader", "create_loaders", None),
    "finetune_locobot": ("src.dataset.locobot.locobot_singleview_dataloader", "create_finetune_loaders", None),
    "train_locobot_table": ("src.dataset.locobot.locobot_table_dataloaders", "create_loaders", None),
}


class Files:
    """Stands in for RoboNetDataset: keeps what it was built from."""

    def __init__(self, files, labels, config, augment_img=False, **kw):
        self.files, self.labels, self.augment = list(files), list(labels), bool(augment_img)


class Loader:
    """Stands in for DataLoader: keeps the dataset and the arguments that decide the batches."""

    def __init__(self, dataset, batch_size=1, shuffle=False, **kw):
        self.dataset, self.batch_size, self.shuffle = dataset, batch_size, shuffle


def module(name):
    mod = importlib.import_module(name)
    mod.RoboNetDataset, mod.DataLoader = Files, Loader
    mod.has_file_allowed_extension = lambda path, ext: path.lower().endswith(ext)
    return mod


def record(loader, root):
    ds = loader.dataset
    return {"files": [os.path.relpath(p, root) for p in ds.files], "labels": ds.labels, "augment": ds.augment,
            "batch_size": loader.batch_size, "shuffle": bool(loader.shuffle)}


def main():
    out = {}
    with tempfile.TemporaryDirectory() as root:
        refs.write_tree(root)
        for experiment in refs.EXPERIMENTS:
            mod, fn, transfer = CHOICE[experiment]
            for seed in refs.SEEDS:
                cf = refs.config(root, experiment, seed, img_augmentation=True)
                train, test = getattr(module(mod), fn)(cf)
                case = {"train": record(train, root), "test": record(test, root), "transfer": None}
                if transfer is not None:
                    case["transfer"] = record(getattr(module(transfer[0]), transfer[1])(cf), root)
                out[refs.case_key(experiment, seed)] = case
    with open(refs.GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote", refs.GOLDEN, os.path.getsize(refs.GOLDEN) // 1024, "KB;",
          {k: (len(v["train"]["files"]), len(v["test"]["files"])) for k, v in out.items()})


if __name__ == "__main__":
    main()
