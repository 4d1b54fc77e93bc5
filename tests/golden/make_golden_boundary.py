"""Build-container-only: two facts of the reference checkout that tests/test_boundary_cpu.py compares the package with.

    offset_keypoint_ptv3_model_cfg.txt  the `model` dict of configs/my_dataset/offset_keypoint_ptv3.py:11-46, as a Python
                                        literal (tuples kept), read with ast.literal_eval
    reference_train_keys.json           the "train/..." keys the reference's offset wrappers put into their training
                                        result (pointcept/models/offset_keypoint_ptv3.py:92-98,
                                        offset_keypoint_swin3d.py:92-124), per file

    python tests/golden/make_golden_boundary.py          (needs the reference checkout; PTV3_REFERENCE_ROOT)
"""
import json
import os
import pprint
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

# the key pattern the test applies to this package's files
TRAIN_KEY = r'\[f?"(train/[a-z0-9_{}]+)"\]'


def main():
    assert ref_loader.available(), "run in the build container (needs the reference checkout)"
    scope = {}
    path = os.path.join(ref_loader.REF, "configs", "my_dataset", "offset_keypoint_ptv3.py")
    exec(compile(open(path).read(), path, "exec"), scope)
    with open(os.path.join(HERE, "offset_keypoint_ptv3_model_cfg.txt"), "w") as f:
        f.write(pprint.pformat(scope["model"], sort_dicts=False, width=100) + "\n")
    models = os.path.join(ref_loader.REF, "pointcept", "models")
    keys = {name: sorted(set(re.findall(TRAIN_KEY, open(os.path.join(models, name)).read())))
            for name in ("offset_keypoint_ptv3.py", "offset_keypoint_swin3d.py")}
    with open(os.path.join(HERE, "reference_train_keys.json"), "w") as f:
        json.dump(keys, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
