"""Box / misc helpers of the ConQueR playground ($CQ/modules/utils.py:16-113,277-314, $CQ/modules/blocks.py)."""
import copy

import torch
import torch.nn.functional as F
from torch import nn

from ..operators.linear import Linear, linear


class MLP(nn.Module):
    """$CQ/modules/blocks.py:5-17: Linear+ReLU stack, no activation on the last layer."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            # hidden layers: Linear + ReLU as one product with a fused epilogue / one-launch backward (operators/linear.py)
            x = linear(x, layer.weight, layer.bias, relu=True) if i < self.num_layers - 1 else layer(x)
        return x


def get_clones(module, n):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(n)])


def inverse_sigmoid(x, eps=1e-5):
    """$CQ/modules/utils.py:83-87."""
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def box_cxcyczlwh_to_xyxyxy(x):
    c, s = x[..., :3], x[..., 3:6]
    return torch.cat((c - 0.5 * s, c + 0.5 * s), dim=-1)


def generalized_box3d_iou(boxes1, boxes2):
    """Axis-aligned 3-D GIoU matrix [N, M] of (x0,y0,z0,x1,y1,z1) boxes ($CQ/modules/utils.py:29-72)."""
    boxes1 = torch.nan_to_num(boxes1)
    boxes2 = torch.nan_to_num(boxes2)
    vol1 = (boxes1[:, 3] - boxes1[:, 0]) * (boxes1[:, 4] - boxes1[:, 1]) * (boxes1[:, 5] - boxes1[:, 2])
    vol2 = (boxes2[:, 3] - boxes2[:, 0]) * (boxes2[:, 4] - boxes2[:, 1]) * (boxes2[:, 5] - boxes2[:, 2])
    lo = torch.max(boxes1[:, None, :3], boxes2[:, :3])
    hi = torch.min(boxes1[:, None, 3:], boxes2[:, 3:])
    lwh = (hi - lo).clamp(min=0)
    inter = lwh[:, :, 0] * lwh[:, :, 1] * lwh[:, :, 2]
    union = vol1[:, None] + vol2 - inter
    iou = inter / union
    lo = torch.min(boxes1[:, None, :3], boxes2[:, :3])
    hi = torch.max(boxes1[:, None, 3:], boxes2[:, 3:])
    whl = (hi - lo).clamp(min=0)
    vol = whl[:, :, 0] * whl[:, :, 1] * whl[:, :, 2]
    return iou - (vol - union) / vol


def pairwise_box3d_giou(boxes1, boxes2):
    """generalized_box3d_iou with leading batch dims: boxes1 [..., N, 6], boxes2 [..., M, 6] -> [..., N, M]."""
    boxes1 = torch.nan_to_num(boxes1)[..., :, None, :]
    boxes2 = torch.nan_to_num(boxes2)[..., None, :, :]
    vol1 = (boxes1[..., 3] - boxes1[..., 0]) * (boxes1[..., 4] - boxes1[..., 1]) * (boxes1[..., 5] - boxes1[..., 2])
    vol2 = (boxes2[..., 3] - boxes2[..., 0]) * (boxes2[..., 4] - boxes2[..., 1]) * (boxes2[..., 5] - boxes2[..., 2])
    lwh = (torch.min(boxes1[..., 3:], boxes2[..., 3:]) - torch.max(boxes1[..., :3], boxes2[..., :3])).clamp(min=0)
    inter = lwh[..., 0] * lwh[..., 1] * lwh[..., 2]
    union = vol1 + vol2 - inter
    whl = (torch.max(boxes1[..., 3:], boxes2[..., 3:]) - torch.min(boxes1[..., :3], boxes2[..., :3])).clamp(min=0)
    vol = whl[..., 0] * whl[..., 1] * whl[..., 2]
    return inter / union - (vol - union) / vol


def paired_box3d_giou(boxes1, boxes2):
    """Row-wise GIoU (the diagonal of generalized_box3d_iou, without building the matrix)."""
    boxes1 = torch.nan_to_num(boxes1)
    boxes2 = torch.nan_to_num(boxes2)
    vol1 = (boxes1[:, 3] - boxes1[:, 0]) * (boxes1[:, 4] - boxes1[:, 1]) * (boxes1[:, 5] - boxes1[:, 2])
    vol2 = (boxes2[:, 3] - boxes2[:, 0]) * (boxes2[:, 4] - boxes2[:, 1]) * (boxes2[:, 5] - boxes2[:, 2])
    lwh = (torch.min(boxes1[:, 3:], boxes2[:, 3:]) - torch.max(boxes1[:, :3], boxes2[:, :3])).clamp(min=0)
    inter = lwh[:, 0] * lwh[:, 1] * lwh[:, 2]
    union = vol1 + vol2 - inter
    whl = (torch.max(boxes1[:, 3:], boxes2[:, 3:]) - torch.min(boxes1[:, :3], boxes2[:, :3])).clamp(min=0)
    vol = whl[:, 0] * whl[:, 1] * whl[:, 2]
    return inter / union - (vol - union) / vol


# ---- heading-aware 3-D GIoU -------------------------------------------------------------------------------------------------
# The plain PyTorch form of rot_giou3d in csrc/giou3d.h (same definition, same pair-local frame): the model's CPU path, the
# EFG_FUSED_LOSS=0 path on the GPU and, in float64, the yardstick of the kernels' tests.  Differentiable by autograd.
def _inside_part(px, py, hx, hy, strict, ox, oy):
    """Green's-theorem share 1/2 sum cross(p0, p1) of the parts of a quadrilateral's four edges that lie inside the centred
    rectangle |x| <= hx, |y| <= hy.  (px, py) [..., 4]: its corners in the rectangle's frame, where the edges are clipped;
    (ox, oy): the same corners in the frame the share is summed in.  strict: an edge parallel to a side and ON it is outside."""
    ex, ey = px.roll(-1, -1) - px, py.roll(-1, -1) - py
    t0, t1 = torch.zeros_like(px), torch.ones_like(px)
    for p, d, h in ((px, ex, hx[..., None]), (py, ey, hy[..., None])):
        par = d == 0
        safe = torch.where(par, torch.ones_like(d), d)
        ta, tb = (-h - p) / safe, (h - p) / safe
        inside = (p.abs() < h) if strict else (p.abs() <= h)
        t0 = torch.where(par, t0, torch.maximum(t0, torch.minimum(ta, tb)))
        t1 = torch.where(par, torch.where(inside, t1, -torch.ones_like(t1)), torch.minimum(t1, torch.maximum(ta, tb)))
    fx, fy = ox.roll(-1, -1) - ox, oy.roll(-1, -1) - oy
    x0, y0, x1, y1 = ox + t0 * fx, oy + t0 * fy, ox + t1 * fx, oy + t1 * fy
    part = torch.where(t1 > t0, 0.5 * (x0 * y1 - y0 * x1), torch.zeros_like(x0))
    return part.sum(-1)


def _hull_area(x, y):
    """Area of the convex hull of the points (x, y) [..., 8]: gift wrapping from the lowest (then leftmost) point, at most 8
    steps, shoelace sum over the steps.  The selection is index arithmetic (no gradient); the gathered vertices carry it."""
    tol = 8 * torch.finfo(x.dtype).eps
    with torch.no_grad():
        low = torch.where(y == y.min(-1, keepdim=True).values, x, torch.full_like(x, float("inf"))).argmin(-1, keepdim=True)
    sx, sy = x.gather(-1, low), y.gather(-1, low)
    cx, cy = sx, sy
    dirx, diry = torch.ones_like(cx).detach(), torch.zeros_like(cy).detach()
    done = torch.zeros_like(cx, dtype=torch.bool)
    area = torch.zeros_like(cx)
    for _ in range(8):
        with torch.no_grad():
            ex, ey = x - cx, y - cy
            # angle from the incoming direction, in [0, pi] (every point is to the left of it); the farthest of collinear ones
            ang = torch.atan2((dirx * ey - diry * ex).clamp(min=0) + 0.0, dirx * ex + diry * ey)
            ang = torch.where((ex == 0) & (ey == 0), torch.full_like(ang, float("inf")), ang)
            tie = ang <= ang.min(-1, keepdim=True).values + tol
            nxt = torch.where(tie, ex * ex + ey * ey, torch.full_like(ang, -1.0)).argmax(-1, keepdim=True)
        nx, ny = x.gather(-1, nxt), y.gather(-1, nxt)
        area = area + torch.where(done, torch.zeros_like(area), 0.5 * (cx * ny - cy * nx))
        with torch.no_grad():
            done = done | ((nx == sx) & (ny == sy))
            dirx, diry = (nx - cx).detach(), (ny - cy).detach()
        cx, cy = nx, ny
    return area[..., 0]


def rot_giou3d(boxes1, boxes2, frame):
    """(GIoU, IoU) of broadcastable 7-DoF boxes (cx, cy, cz, l, w, h, rad) [..., 7]: rotated-rectangle intersection and convex
    hull in the bird's-eye view times the z overlap / z range.  frame = (sx, sy, yaw_scale, yaw_offset): metric centre
    (cx sx, cy sy), size (l sx, w sy), yaw = rad yaw_scale + yaw_offset.  All planar geometry is evaluated in the frame of the
    second box (origin at its centre, axes along its sides)."""
    sx, sy, ys, yo = (float(v) for v in frame)
    a, b = torch.broadcast_tensors(torch.nan_to_num(boxes1), torch.nan_to_num(boxes2))
    al, aw, bl, bw = a[..., 3] * sx, a[..., 4] * sy, b[..., 3] * sx, b[..., 4] * sy
    hax, hay, hbx, hby = 0.5 * al, 0.5 * aw, 0.5 * bl, 0.5 * bw
    ddx, ddy = (a[..., 0] - b[..., 0]) * sx, (a[..., 1] - b[..., 1]) * sy
    yaw_b, theta = b[..., 6] * ys + yo, (a[..., 6] - b[..., 6]) * ys
    cb, sb, ct, st = torch.cos(yaw_b), torch.sin(yaw_b), torch.cos(theta)[..., None], torch.sin(theta)[..., None]
    dx, dy = (cb * ddx + sb * ddy)[..., None], (cb * ddy - sb * ddx)[..., None]
    su, sv = a.new_tensor([1.0, -1.0, -1.0, 1.0]), a.new_tensor([1.0, 1.0, -1.0, -1.0])   # counter-clockwise corners
    ax = dx + su * hax[..., None] * ct - sv * hay[..., None] * st
    ay = dy + su * hax[..., None] * st + sv * hay[..., None] * ct
    bx, by = su * hbx[..., None], sv * hby[..., None]
    # intersection: the parts of A's edges inside the closed B and of B's edges inside the open A (edges lying on each other
    # count once), summed in B's frame
    rx, ry = ct * (bx - dx) + st * (by - dy), ct * (by - dy) - st * (bx - dx)
    inter = (_inside_part(ax, ay, hbx, hby, False, ax, ay) + _inside_part(rx, ry, hax, hay, True, bx, by)).clamp(min=0)
    hull = _hull_area(torch.cat((ax, bx), -1), torch.cat((ay, by), -1)).clamp(min=0)
    alo, ahi, blo, bhi = a[..., 2] - 0.5 * a[..., 5], a[..., 2] + 0.5 * a[..., 5], b[..., 2] - 0.5 * b[..., 5], b[..., 2] + 0.5 * b[..., 5]
    z_overlap = (torch.minimum(ahi, bhi) - torch.maximum(alo, blo)).clamp(min=0)
    z_range = (torch.maximum(ahi, bhi) - torch.minimum(alo, blo)).clamp(min=0)
    inter3d = inter * z_overlap
    union3d = al * aw * a[..., 5] + bl * bw * b[..., 5] - inter3d
    hull3d = hull * z_range
    iou = inter3d / union3d
    return iou - (hull3d - union3d) / hull3d, iou


def paired_rot_giou3d(boxes1, boxes2, frame):
    """Row-wise heading-aware GIoU of boxes1 [N, 7] and boxes2 [N, 7] -> [N]."""
    return rot_giou3d(boxes1, boxes2, frame)[0]


def pairwise_rot_giou3d(boxes1, boxes2, frame):
    """Heading-aware GIoU matrix: boxes1 [..., N, 7], boxes2 [..., M, 7] -> [..., N, M]."""
    return rot_giou3d(boxes1[..., :, None, :], boxes2[..., None, :, :], frame)[0]


def sigmoid_focal_loss(logits, targets, alpha=-1.0, gamma=2.0, reduction="none"):
    """efg/modeling/losses/focal_loss.py:5-45."""
    p = torch.sigmoid(logits)
    ce_loss = F.binary_cross_entropy_with_logits(logits, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce_loss * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    return loss


_SHAPES = {}


def _shapes_on_device(shapes, device):
    """int64 [N,2] level shapes on `device`, built once per distinct shape set: torch.tensor(list, device=...)
    is a SYNCHRONOUS upload -- it waits for everything queued on the stream (the previous step's backward)."""
    key = (shapes, str(device))
    if key not in _SHAPES:
        _SHAPES[key] = torch.tensor(shapes, dtype=torch.int64).to(device)
    return _SHAPES[key]


def flatten_with_shape(tensor_list):
    """[(B,C,Hi,Wi)] -> ((B, sum Hi*Wi, C), int64 [N,2] shapes) ($CQ/modules/utils.py:277-314)."""
    shapes = _shapes_on_device(tuple((t.shape[2], t.shape[3]) for t in tensor_list), tensor_list[0].device)
    if len(tensor_list) == 1:  # one level: a channels-last map already IS the token layout (cat would copy it)
        flat = tensor_list[0].flatten(2).permute(0, 2, 1).contiguous()
    else:
        flat = torch.cat([t.flatten(2).permute(0, 2, 1) for t in tensor_list], dim=1)
    return flat, shapes


def limit_period(val, offset=0.5, period=3.141592653589793):
    """efg/geometry/box_ops_torch.py:229-241."""
    return val - torch.floor(val / period + offset) * period
