"""Writes tests/golden/augment_parent.npz: what augment.sample_params / affine_matrices returned BEFORE the mirror and
colour options existed, on the parameter sets of tests/test_augment_cpu.py.  tests/test_augment_jitter_cpu.py holds the
sampler to these bits with the options off.  It was run once, on the commit in front of the options (d2ac4eb); running it
on a later commit only shows that nothing moved.

    python tests/golden/make_augment_parent.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# (name, seed, step, src_hw rows, out_hw, mode): the sample_params calls of tests/test_augment_cpu.py (the 1000-image and
# 200-step ones cut to 60 images and 20 steps)
SAMPLED = [
    ("keyed", 7, 3, [[200, 300], [480, 640], [17, 23]], (384, 384), "train"),
    ("ranges", 1, 0, [[211, 317]] * 60, (384, 384), "train"),
    ("inverse", 3, 1, [[200, 300], [97, 61]] * 50, (384, 384), "train"),
    ("val", 5, 9, [[200, 300], [48, 64]], (96, 128), "val"),
] + [(f"blob{step}", 11, step, [[120, 160]], (96, 128), "train") for step in range(20)]
# (name, theta, scale, crop, src_hw, out_hw): its direct affine_matrices calls
DIRECT = [
    ("identity", 0.0, 1.0, (0, 0, 0, 0), (24, 40), (24, 40)),
    ("rot180", 180.0, 1.0, (0, 0, 0, 0), (17, 23), (17, 23)),
    ("zoom", 0.0, 2.5, (0, 0, 0, 0), (40, 40), (40, 40)),
]


def main():
    from pytorch_pose_proposal_network_amd import augment as A
    out = {}
    for name, seed, step, hw, out_hw, mode in SAMPLED:
        hw = np.asarray(hw, np.int32)
        p = A.sample_params(seed, step, hw, out_hw, mode)
        f64 = A.affine_matrices(p["theta"], p["scale"], p["crop"], hw, out_hw)
        for k in ("theta", "scale", "crop", "fwd", "inv"):
            out[f"{name}/{k}"] = p[k]
        out[f"{name}/fwd64"], out[f"{name}/inv64"] = f64
    for name, theta, scale, crop, hw, out_hw in DIRECT:
        out[f"{name}/fwd64"], out[f"{name}/inv64"] = A.affine_matrices(theta, scale, crop, hw, out_hw)
    np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "augment_parent.npz"), **out)


if __name__ == "__main__":
    main()
