"""tests/golden/rot_giou_ref.npz: the reference's own heading-aware 3-D GIoU (efg/modeling/losses/iou3d_loss.py
generalized_box_iou3d, imported in place from the reference tree) and its autograd gradient on 500 random pairs near the
origin and on the same pairs moved by (70, 70) m.

    python scripts/make_golden_rot_giou.py <reference tree> [output.npz]

The reference allocates float32 internally and fails on float64 inputs: it is run in float32, which is what its numbers are
(tests/test_rot_giou_ref.py holds the PyTorch formulation of this package to them within 5e-5 on the near family).
Boxes are metric (x, y, z, l, w, h, yaw); the reference reads (x, y, z, l, w, h, cos yaw, sin yaw), built here from a leaf yaw
so that the gradient comes back for the seven parameters of the first box."""
import importlib.util
import os
import sys

import numpy as np
import torch

N_PAIRS, SHIFT, SEED = 500, 70.0, 20240607


def random_boxes(rng, n):
    """centres within +-1.5 m (z within +-1 m), l in [0.5, 6], w, h in [0.5, 3], yaw uniform in (-pi, pi)"""
    b = np.empty((n, 7), dtype=np.float64)
    b[:, :2] = rng.uniform(-1.5, 1.5, (n, 2))
    b[:, 2] = rng.uniform(-1.0, 1.0, n)
    b[:, 3] = rng.uniform(0.5, 6.0, n)
    b[:, 4:6] = rng.uniform(0.5, 3.0, (n, 2))
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b.astype(np.float32)


def reference_giou_and_grad(mod, a, b):
    a7 = torch.from_numpy(a).clone().requires_grad_(True)
    b7 = torch.from_numpy(b)

    def eight(x):
        return torch.cat((x[:, :6], torch.cos(x[:, 6:7]), torch.sin(x[:, 6:7])), dim=1)

    giou = mod.generalized_box_iou3d(eight(a7), eight(b7))
    grad, = torch.autograd.grad(giou.sum(), a7)
    return giou.detach().numpy(), grad.numpy()


def main():
    ref_root = sys.argv[1]
    here = os.path.dirname(os.path.abspath(__file__))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "..", "tests", "golden", "rot_giou_ref.npz")
    spec = importlib.util.spec_from_file_location("ref_iou3d_loss", os.path.join(ref_root, "efg/modeling/losses/iou3d_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(SEED)
    a_near, b_near = random_boxes(rng, N_PAIRS), random_boxes(rng, N_PAIRS)
    shift = np.zeros(7, dtype=np.float32)
    shift[:2] = SHIFT
    a_far, b_far = a_near + shift, b_near + shift
    giou_near, grad_near = reference_giou_and_grad(mod, a_near, b_near)
    giou_far, grad_far = reference_giou_and_grad(mod, a_far, b_far)
    np.savez_compressed(out, a_near=a_near, b_near=b_near, a_far=a_far, b_far=b_far, giou_near=giou_near, giou_far=giou_far,
                        grad_near=grad_near, grad_far=grad_far, shift=np.float32(SHIFT), seed=np.int64(SEED))
    print(out, os.path.getsize(out), "bytes; giou near [%.3f, %.3f]" % (giou_near.min(), giou_near.max()))


if __name__ == "__main__":
    main()
