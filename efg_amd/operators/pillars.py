"""PointPillars reader on the device (csrc/pillars.hip).

`pillar_features(voxels, num_points, coors, weight, bn, ...)` is the one-layer PillarFeatureNet of
efg/modeling/readers/pillar_encoder.py:98-132 -- decorate, Linear(Cin, 64, bias=False), BatchNorm1d, ReLU, max over the
pillar's rows -- as two passes over the points (statistics, apply) in training mode and one in eval mode; nothing of shape
[P, N, C] is written.  The forward saves the arg-max row (uint8), mean and rstd; the backward is one more pass plus a finishing
launch and returns the gradients of the Linear weight and the BatchNorm affine (the points are data).
`pillar_scatter(features, coors, batch_size, nx, ny)` is PointPillarsScatter (:149-184) into a channels-last canvas; its
backward is the row gather.  Every sum has a fixed order: two runs agree in every bit.

Precondition: every pillar has num_points >= 1 (the voxelizer guarantees it) and coordinates inside the grid."""
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib as L

CHANNELS = 64        # output channels of the fused layer: the lanes of a wave
MAX_ROWS = 64        # N
MAX_CIN = 16
MIN_FEATURES = 3


def _workspace(dev):
    nbytes = L.lib().efg_pillar_workspace_bytes()
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _check_limits(voxels, weight, with_distance):
    """Raise before anything is launched; nothing is truncated."""
    if voxels.dim() != 3:
        raise ValueError("pillar_features: voxels must be [P, N, F], got %s" % (tuple(voxels.shape),))
    _, n, f = voxels.shape
    cin = f + 5 + (1 if with_distance else 0)
    if tuple(weight.shape) != (CHANNELS, cin):
        raise ValueError("pillar_features: the fused layer is Linear(%d, %d); the weight is %s"
                         % (cin, CHANNELS, tuple(weight.shape)))
    if not 1 <= n <= MAX_ROWS:
        raise ValueError("pillar_features: N = %d rows per pillar, the fused layer takes 1..%d" % (n, MAX_ROWS))
    if f < MIN_FEATURES or cin > MAX_CIN:
        raise ValueError("pillar_features: F = %d raw features (Cin = %d), the fused layer takes F >= %d and Cin <= %d"
                         % (f, cin, MIN_FEATURES, MAX_CIN))


class PillarFeaturesFunction(Function):
    @staticmethod
    def forward(ctx, voxels, num_points, coors, weight, gamma, beta, running_mean, running_var, num_batches_tracked,
                momentum, eps, batch_stats, vx, vy, x_offset, y_offset, with_distance, max_blocks):
        voxels, weight = voxels.contiguous(), weight.contiguous()
        if voxels.data_ptr() % 16:       # a slice of a larger batch: the kernels stage tiles with 16-byte loads
            voxels = voxels.clone()
        num_points = num_points.to(torch.int32).contiguous()
        coors = coors.to(torch.int32).contiguous()
        p, n, f = voxels.shape
        dev = voxels.device
        out = torch.empty((p, CHANNELS), dtype=torch.float32, device=dev)
        index = torch.empty((p, CHANNELS), dtype=torch.uint8, device=dev)
        if batch_stats:
            mean = torch.empty(CHANNELS, dtype=torch.float32, device=dev)
            rstd = torch.empty(CHANNELS, dtype=torch.float32, device=dev)
        else:   # eval mode: the running statistics
            mean = running_mean.detach().clone()
            rstd = 1.0 / torch.sqrt(running_var.detach() + eps)
        if p > 0:
            ws, ws_bytes = _workspace(dev)
            track = batch_stats and running_mean is not None
            L.check(L.lib().efg_pillar_forward_f32(
                L.ptr(voxels), L.ptr(num_points), L.ptr(coors), L.ptr(weight), L.ptr(gamma), L.ptr(beta),
                L.ptr(running_mean) if track else None, L.ptr(running_var) if track else None,
                L.ptr(num_batches_tracked) if track else None, float(momentum) if track else 0.0, float(eps), p, n, f,
                1 if with_distance else 0, CHANNELS, float(vx), float(vy), float(x_offset), float(y_offset),
                1 if batch_stats else 0, L.ptr(mean), L.ptr(rstd), L.ptr(out), L.ptr(index), L.ptr(ws), ws_bytes,
                int(max_blocks), L.stream()))
        ctx.save_for_backward(voxels, num_points, coors, weight, gamma, beta, mean, rstd, index)
        ctx.geometry = (float(vx), float(vy), float(x_offset), float(y_offset), bool(with_distance), bool(batch_stats),
                        int(max_blocks))
        ctx.mark_non_differentiable(index, *[t for t in (running_mean, running_var, num_batches_tracked) if t is not None])
        return out, index

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, _dindex):
        voxels, num_points, coors, weight, gamma, beta, mean, rstd, index = ctx.saved_tensors
        vx, vy, x_offset, y_offset, with_distance, batch_stats, max_blocks = ctx.geometry
        p, n, f = voxels.shape
        dev = voxels.device
        if p == 0:
            return (None, None, None, torch.zeros_like(weight), torch.zeros_like(gamma), torch.zeros_like(beta)) + (None,) * 12
        dy = dy.contiguous()
        dweight = torch.empty_like(weight)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        ws, ws_bytes = _workspace(dev)
        L.check(L.lib().efg_pillar_backward_f32(
            L.ptr(voxels), L.ptr(num_points), L.ptr(coors), L.ptr(weight), L.ptr(gamma), L.ptr(beta), L.ptr(mean),
            L.ptr(rstd), L.ptr(dy), L.ptr(index), p, n, f, 1 if with_distance else 0, CHANNELS, vx, vy, x_offset, y_offset,
            1 if batch_stats else 0, L.ptr(dweight), L.ptr(dgamma), L.ptr(dbeta), L.ptr(ws), ws_bytes, max_blocks,
            L.stream()))
        return (None, None, None, dweight, dgamma, dbeta) + (None,) * 12


def usable(voxels, weight, bn, with_distance=False):
    """Whether the fused layer covers this call: a GPU fp32 [P, N <= 64, F] batch, Linear(F + 5 (+ 1) <= 16, 64), an affine
    BatchNorm1d with a fixed momentum.  Anything else is the PyTorch composition (modeling/readers/pillar_encoder.py)."""
    if os.environ.get("EFG_FUSED_PILLARS", "1") == "0":
        return False
    if not (voxels.is_cuda and voxels.dtype == torch.float32 and voxels.dim() == 3 and weight.is_cuda
            and weight.dtype == torch.float32 and weight.dim() == 2):
        return False
    if type(bn) is not torch.nn.BatchNorm1d or not bn.affine or bn.weight.dtype != torch.float32:
        return False
    if bn.track_running_stats and bn.momentum is None:      # the cumulative average is not built
        return False
    _, n, f = voxels.shape
    cin = f + 5 + (1 if with_distance else 0)
    return (tuple(weight.shape) == (CHANNELS, cin) and bn.num_features == CHANNELS and 1 <= n <= MAX_ROWS
            and f >= MIN_FEATURES and cin <= MAX_CIN)


def pillar_features(voxels, num_points, coors, weight, bn, vx, vy, x_offset, y_offset, with_distance=False,
                    return_index=False, max_blocks=0):
    """max_n relu(bn(Linear(decorate(voxels)))) -> [P, 64] (and the arg-max row, uint8 [P, 64], with `return_index`).

    voxels [P, N, F] fp32, num_points [P] (>= 1), coors [P, 4] (b, z, y, x), weight [64, F + 5 (+ 1)], `bn` an affine
    nn.BatchNorm1d(64): in training mode (or without running statistics) the batch statistics over the P * N rows are
    used and the running statistics updated; in eval mode the running ones.  GPU tensors only; limits raise."""
    L.require_gpu(voxels, num_points, coors, weight, bn.weight)
    _check_limits(voxels, weight, with_distance)
    if type(bn) is not torch.nn.BatchNorm1d or not bn.affine:
        raise ValueError("pillar_features: needs an affine nn.BatchNorm1d")
    if bn.track_running_stats and bn.momentum is None:
        raise ValueError("pillar_features: BatchNorm1d(momentum=None) is not supported by the fused layer")
    batch_stats = bn.training or not bn.track_running_stats
    tracked = bn.track_running_stats
    out, index = PillarFeaturesFunction.apply(
        voxels, num_points, coors, weight, bn.weight, bn.bias, bn.running_mean if tracked else None,
        bn.running_var if tracked else None, bn.num_batches_tracked if tracked else None, bn.momentum, bn.eps, batch_stats,
        vx, vy, x_offset, y_offset, with_distance, max_blocks)
    return (out, index) if return_index else out


class PillarScatterFunction(Function):
    @staticmethod
    def forward(ctx, features, coors, batch_size, nx, ny):
        features = features.contiguous()
        coors = coors.to(torch.int32).contiguous()
        p, c = features.shape
        # [B, ny, nx, C] row-major IS the channels-last memory of a [B, C, ny, nx] map
        canvas = torch.zeros((batch_size, ny, nx, c), dtype=features.dtype, device=features.device).permute(0, 3, 1, 2)
        if p > 0:
            L.check(L.lib().efg_pillar_scatter_f32(L.ptr(features), L.ptr(coors), p, c, batch_size, ny, nx,
                                                   canvas.data_ptr(), L.stream()))
        ctx.save_for_backward(coors)
        ctx.shape = (p, c, batch_size, ny, nx)
        return canvas

    @staticmethod
    @once_differentiable
    def backward(ctx, dcanvas):
        coors, = ctx.saved_tensors
        p, c, batch_size, ny, nx = ctx.shape
        dcanvas = dcanvas.contiguous(memory_format=torch.channels_last)
        dfeat = torch.empty((p, c), dtype=dcanvas.dtype, device=dcanvas.device)
        if p > 0:
            L.check(L.lib().efg_pillar_gather_f32(dcanvas.data_ptr(), L.ptr(coors), p, c, batch_size, ny, nx,
                                                  L.ptr(dfeat), L.stream()))
        return dfeat, None, None, None, None


def pillar_scatter(features, coors, batch_size, nx, ny):
    """canvas[b, :, y, x] = features[p] for coors[p] = (b, z, y, x): a zero-filled [B, C, ny, nx] in channels-last
    memory.  Pillar coordinates are unique per scene."""
    L.require_gpu(features, coors)
    if features.dim() != 2 or features.dtype != torch.float32:
        raise ValueError("pillar_scatter: features must be fp32 [P, C], got %s %s" % (features.dtype, tuple(features.shape)))
    if coors.shape != (features.shape[0], 4):
        raise ValueError("pillar_scatter: coors must be [P, 4], got %s" % (tuple(coors.shape),))
    if batch_size < 1 or nx < 1 or ny < 1:
        raise ValueError("pillar_scatter: batch %d, canvas %d x %d" % (batch_size, ny, nx))
    return PillarScatterFunction.apply(features, coors, int(batch_size), int(nx), int(ny))
