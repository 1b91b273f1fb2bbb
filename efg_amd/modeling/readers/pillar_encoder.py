"""PointPillars reader and its BEV scatter (reference: efg/modeling/readers/pillar_encoder.py, same class, parameter and
buffer names -- `pfn_layers.i.linear.weight`, `pfn_layers.i.norm.*` -- so its state dicts load with strict=True).

On GPU tensors a net of ONE layer with 64 output channels, Cin = num_input_features + 5 (+ 1) <= 16 and N <= 64 rows per
pillar runs as the fused kernels of csrc/pillars.hip (operators/pillars.py); everything else -- CPU tensors, more layers,
other widths, another norm -- runs the PyTorch composition of the reference's lines, `forward_composition`.

Precondition: every pillar holds at least one point (num_voxels >= 1; the voxelizer guarantees it)."""
import torch
from torch import nn
from torch.nn import functional as F

from ...operators import pillars as pillar_ops
from ..common import get_norm


def get_paddings_indicator(actual_num, max_num, axis=0):
    """[P, max_num] bool: row n of pillar p is a point (efg/modeling/utils.py:156-174)."""
    actual_num = torch.unsqueeze(actual_num, axis + 1)
    shape = [1] * len(actual_num.shape)
    shape[axis + 1] = -1
    rows = torch.arange(max_num, dtype=torch.int, device=actual_num.device).view(shape)
    return actual_num.int() > rows


class PFNLayer(nn.Module):
    def __init__(self, in_channels, out_channels, norm="BN1d", last_layer=False):
        super().__init__()
        self.last_vfe = last_layer
        if not self.last_vfe:
            out_channels = out_channels // 2
        self.units = out_channels
        self.linear = nn.Linear(in_channels, self.units, bias=False)
        self.norm = get_norm(norm, self.units)

    def forward(self, inputs):
        x = self.linear(inputs)
        x = self.norm(x.permute(0, 2, 1).contiguous()).permute(0, 2, 1).contiguous()
        x = F.relu(x)
        x_max = torch.max(x, dim=1, keepdim=True)[0]
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max.repeat(1, inputs.shape[1], 1)], dim=2)


class PillarFeatureNet(nn.Module):
    def __init__(self, num_input_features=4, num_filters=(64,), with_distance=False, voxel_size=(0.2, 0.2, 4),
                 pc_range=(0, -40, -3, 70.4, 40, 1), norm="BN1d"):
        super().__init__()
        assert len(num_filters) > 0
        self.num_input = num_input_features
        num_input_features += 5
        if with_distance:
            num_input_features += 1
        self._with_distance = with_distance
        num_filters = [num_input_features] + list(num_filters)
        self.pfn_layers = nn.ModuleList(
            [PFNLayer(num_filters[i], num_filters[i + 1], norm=norm, last_layer=i == len(num_filters) - 2)
             for i in range(len(num_filters) - 1)])
        # x / y offset of a pillar's centre, evaluated on the host as in the reference
        self.vx = voxel_size[0]
        self.vy = voxel_size[1]
        self.x_offset = self.vx / 2 + pc_range[0]
        self.y_offset = self.vy / 2 + pc_range[1]

    def usable(self, features):
        """The fused kernels cover this call (operators/pillars.py:usable)."""
        return (len(self.pfn_layers) == 1 and features.dim() == 3
                and pillar_ops.usable(features, self.pfn_layers[0].linear.weight, self.pfn_layers[0].norm,
                                      self._with_distance))

    def decorate(self, features, num_voxels, coors):
        """[P, N, F] -> [P, N, F + 5 (+ 1)], rows past the count zeroed (pillar_encoder.py:101-126)."""
        dtype = features.dtype
        points_mean = features[:, :, :3].sum(dim=1, keepdim=True) / num_voxels.type_as(features).view(-1, 1, 1)
        f_cluster = features[:, :, :3] - points_mean
        f_center = torch.zeros_like(features[:, :, :2])
        f_center[:, :, 0] = features[:, :, 0] - (coors[:, 3].to(dtype).unsqueeze(1) * self.vx + self.x_offset)
        f_center[:, :, 1] = features[:, :, 1] - (coors[:, 2].to(dtype).unsqueeze(1) * self.vy + self.y_offset)
        features_ls = [features, f_cluster, f_center]
        if self._with_distance:
            features_ls.append(torch.norm(features[:, :, :3], 2, 2, keepdim=True))
        features = torch.cat(features_ls, dim=-1)
        mask = get_paddings_indicator(num_voxels, features.shape[1], axis=0)
        # where, not `*= mask`: a padded row is zero whatever it holds (inf or NaN included)
        return torch.where(mask.unsqueeze(-1), features, torch.zeros((), dtype=dtype, device=features.device))

    def forward_composition(self, features, num_voxels, coors):
        features = self.decorate(features, num_voxels, coors)
        for pfn in self.pfn_layers:
            features = pfn(features)
        return features.squeeze()

    def forward(self, features, num_voxels, coors):
        if not self.usable(features):
            return self.forward_composition(features, num_voxels, coors)
        layer = self.pfn_layers[0]
        out = pillar_ops.pillar_features(features, num_voxels, coors, layer.linear.weight, layer.norm, self.vx, self.vy,
                                         self.x_offset, self.y_offset, self._with_distance)
        return out.squeeze()        # the reference's [P, 1, 64].squeeze(): [P, 64], or [64] for a single pillar


class PointPillarsScatter(nn.Module):
    def __init__(self, num_input_features=64, norm="BN1d", **kwargs):
        super().__init__()
        self.nchannels = num_input_features

    def forward(self, voxel_features, coords, batch_size, input_shape):
        """-> [B, C, ny, nx] with nx, ny = input_shape[0], input_shape[1]; channels-last memory on the GPU path."""
        if voxel_features.is_cuda and voxel_features.dtype == torch.float32 and voxel_features.dim() == 2:
            self.nx, self.ny = input_shape[0], input_shape[1]
            return pillar_ops.pillar_scatter(voxel_features, coords, batch_size, self.nx, self.ny)
        return self.forward_composition(voxel_features, coords, batch_size, input_shape)

    def forward_composition(self, voxel_features, coords, batch_size, input_shape):
        self.nx = input_shape[0]
        self.ny = input_shape[1]
        batch_canvas = []
        for b in range(batch_size):
            canvas = torch.zeros(self.nchannels, self.nx * self.ny, dtype=voxel_features.dtype, device=voxel_features.device)
            batch_mask = coords[:, 0] == b
            this_coords = coords[batch_mask, :]
            indices = (this_coords[:, 2] * self.nx + this_coords[:, 3]).type(torch.long)
            canvas[:, indices] = voxel_features[batch_mask, :].t()
            batch_canvas.append(canvas)
        return torch.stack(batch_canvas, 0).view(batch_size, self.nchannels, self.ny, self.nx)
