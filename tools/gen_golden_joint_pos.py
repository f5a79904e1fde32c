"""TEST INFRASTRUCTURE ONLY -- golden vectors of the joint-position dataset (`src/dataset/joint_pos_dataset.py`).

Runs only where the reference checkout is present: it loads oracle/gen_golden.py for its recipe (absent third-party
modules stubbed, the reference first on sys.path so that the name `src` is the reference's), imports the REFERENCE's own
`JointPosDataset` with `h5py.File` backed by this package's `.npz` reader and the image transform stubbed (the masks
are pinned by a restatement in the test, not here), and runs it over the seeded trajectories of
tests/joint_pos_oracle.py with `--preprocess_action raw` and `state_infer`.  It records numbers only -- per strategy and
trajectory the item's `states`, `actions`, `qpos` and the window start -- to tests/golden/joint_pos_data.npz.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_joint_pos.py
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


gg = _load("gen_golden", os.path.join(REPO, "oracle", "gen_golden.py"))  # stubs + sys.path: the reference imports now
jpo = _load("joint_pos_oracle", os.path.join(REPO, "tests", "joint_pos_oracle.py"))

for name in ("tqdm",):
    try:
        __import__(name)
    except ImportError:
        gg.MISSING.add(name)

import src.dataset.joint_pos_dataset as ref_mod  # noqa: E402


class NpzFile:
    """An `.npz` archive behind the part of h5py.File the dataset uses: `[name]` with `.shape` and slicing, `.attrs`."""

    def __init__(self, path, mode="r"):
        self._z = np.load(path, allow_pickle=False)
        self.attrs = {k[5:]: str(self._z[k]) for k in self._z.files if k.startswith("attr_")}

    def __getitem__(self, k):
        return self._z[k]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self._z.close()


def main():
    ref_mod.h5py.File = NpzFile
    ref_mod.tf.Compose = lambda transforms: (lambda image: torch.zeros(1))  # masks: not recorded
    out = {}
    with tempfile.TemporaryDirectory() as root:
        paths = jpo.write_root(root)
        names = [os.path.relpath(p, root) for p in paths]
        stored = [np.load(p)["qpos"].astype(np.float32) for p in paths]
        for strategy in ("raw", "state_infer"):
            ds = ref_mod.JointPosDataset(names, ["widowx"] * len(names), jpo.config(root, preprocess_action=strategy))
            for i in range(len(names)):
                item = ds[i]
                for k in ("states", "actions", "qpos"):
                    out[f"{strategy}_{i}_{k}"] = np.asarray(item[k])
                first = np.asarray(item["qpos"])[0]
                (hits,) = np.nonzero((stored[i] == first).all(1))  # the window start, from the item itself
                assert len(hits) == 1, hits
                out[f"{strategy}_{i}_start"] = np.int64(hits[0])
    gg.save("joint_pos_data", **out)
    print("recorded", len(out), "arrays; starts", [int(out[f"raw_{i}_start"]) for i in range(len(jpo.SPECS))])


if __name__ == "__main__":
    main()
