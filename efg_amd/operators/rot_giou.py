"""Heading-aware 3-D GIoU over libefg_hip.so (csrc/rot_giou.hip): one launch forward, one backward.  The PyTorch form of
the same definition is detection3d.utils.rot_giou3d."""
import ctypes
import math

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib as L

METRIC_FRAME = (1.0, 1.0, 1.0, 0.0)


def code_frame(pc_size_x, pc_size_y):
    """The frame of the ConQueR box codes (VoxelBoxCoder3D): centre and size in units of the point-cloud range, yaw
    = rad * 2 pi - pi."""
    return (float(pc_size_x), float(pc_size_y), 2.0 * math.pi, -math.pi)


def frame_arg(frame):
    """(sx, sy, yaw_scale, yaw_offset) as the host float[4] the entry points read."""
    if len(frame) != 4:
        raise ValueError("a box frame is (sx, sy, yaw_scale, yaw_offset), got %r" % (frame,))
    return (ctypes.c_float * 4)(*[float(v) for v in frame])


class RotGIoUPaired(Function):
    """boxes a, b [n, 7] (cx, cy, cz, l, w, h, rad), frame (sx, sy, yaw_scale, yaw_offset) -> (giou [n], iou [n]).  The
    gradient flows through giou; iou is a by-product without one."""

    @staticmethod
    def forward(ctx, a, b, frame):
        L.require_gpu(a, b)
        assert a.shape == b.shape and a.dim() == 2 and a.shape[1] == 7, "RotGIoUPaired: boxes are [n, 7]"
        a32, b32 = a.contiguous().float(), b.contiguous().float()
        n = a32.shape[0]
        giou = torch.empty(n, dtype=torch.float32, device=a.device)
        iou = torch.empty(n, dtype=torch.float32, device=a.device)
        L.check(L.lib().efg_rot_giou_paired_forward_f32(L.ptr(a32), L.ptr(b32), n, frame_arg(frame), L.ptr(giou), L.ptr(iou),
                                                        L.stream()))
        ctx.save_for_backward(a32, b32)
        ctx.frame = tuple(float(v) for v in frame)
        ctx.mark_non_differentiable(iou)
        return giou, iou

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_giou, _grad_iou):
        a32, b32 = ctx.saved_tensors
        ga = torch.empty_like(a32)
        gb = torch.empty_like(b32) if ctx.needs_input_grad[1] else None
        L.check(L.lib().efg_rot_giou_paired_backward_f32(L.ptr(a32), L.ptr(b32), a32.shape[0], frame_arg(ctx.frame),
                                                         L.ptr(grad_giou.contiguous().float()), L.ptr(ga), L.ptr(gb),
                                                         L.stream()))
        return (ga if ctx.needs_input_grad[0] else None), gb, None


def rot_giou_paired(a, b, frame=METRIC_FRAME):
    """(giou, iou) of the rows of a and b [n, 7] on the GPU."""
    return RotGIoUPaired.apply(a, b, tuple(frame))
