"""CenterPoint-PointPillars: PillarFeatureNet -> PointPillarsScatter -> RPN -> CenterHead, the pillar flavour of the detector
of centerpoint/voxelnet.py with the same contract: `forward(batched_inputs)` takes a list of `(sample, info)` pairs -- samples
in the reference format (`voxels`, `num_points_per_voxel`, `coordinates`, `shape`, `range`, `size` from the host pipeline) or
with raw `points` [N, F] on the GPU, voxelized for the whole batch in one call without the per-voxel mean -- and returns the loss
dict in training mode, `CenterHead.predict`'s per-scene detections otherwise.

The reference ships the modules (efg/modeling/readers/pillar_encoder.py) but no pillar experiment, so there is no YAML here
either.  Configuration keys read: `model.reader` -> PillarFeatureNet(**...) (num_input_features, num_filters,
with_distance, voxel_size, pc_range, norm), `model.backbone` -> PointPillarsScatter(**...) (num_input_features), and VoxelNet's
own: `model.neck`, `model.head`, `model.loss`, `model.post_process`, `model.device`, `dataset.pc_range`, `dataset.voxel_size`,
`dataset.processors.{train,val}.Voxelization` (pc_range, voxel_size, max_points_in_voxel, max_voxel_num).  The grid has one
cell in z: voxel_size[2] spans the range."""
import numpy as np
import torch

from ..modeling.readers import PillarFeatureNet, PointPillarsScatter
from ..operators import voxelize_batch
from ..operators.voxelize import wait_for_points
from .voxelnet import VoxelNet


class PointPillars(VoxelNet):
    def _build_reader_and_backbone(self, config):
        self.reader = PillarFeatureNet(**config.model.reader)
        self.backbone = PointPillarsScatter(**config.model.backbone)

    def _inputs(self, samples):
        """-> ((voxels [P, N, F], points per pillar [P]), coordinates [P, 4], batch size, grid (x, y, z), pc_range, voxel_size)"""
        if "voxels" in samples[0]:  # reference format: voxelized on the host by the data pipeline
            voxels = torch.as_tensor(np.concatenate([s["voxels"] for s in samples], 0)).to(self.device)
            npv = torch.as_tensor(np.concatenate([s["num_points_per_voxel"] for s in samples], 0)).to(self.device)
            coors = torch.as_tensor(np.concatenate(
                [np.pad(s["coordinates"], ((0, 0), (1, 0)), mode="constant", constant_values=i)
                 for i, s in enumerate(samples)], 0)).to(self.device)
            return ((voxels, npv), coors, len(samples), list(samples[0]["shape"]), samples[0]["range"], samples[0]["size"])
        vc = self._vox_cfg["train" if self.training else "val"]
        pts = [torch.as_tensor(s["points"], dtype=torch.float32).to(self.device, non_blocking=True) for s in samples]
        geo = self._geometry_stream()
        if geo is None:
            out = voxelize_batch(pts, vc.voxel_size, vc.pc_range, vc.max_points_in_voxel, vc.max_voxel_num, with_mean=False)
        else:
            main = torch.cuda.current_stream()
            wait_for_points(geo, main, samples, pts)
            with torch.cuda.stream(geo):
                out = voxelize_batch(pts, vc.voxel_size, vc.pc_range, vc.max_points_in_voxel, vc.max_voxel_num, with_mean=False)
            main.wait_stream(geo)
            for t in (out["voxels"], out["num_points_per_voxel"], out["coordinates"]):
                t.record_stream(main)
        nf = self.reader.num_input
        voxels = out["voxels"] if out["voxels"].shape[2] == nf else out["voxels"][:, :, :nf].contiguous()
        return ((voxels, out["num_points_per_voxel"]), out["coordinates"], len(samples), self.grid_size, list(vc.pc_range),
                list(vc.voxel_size))

    def _bev(self, feats, coors, batch_size, grid):
        voxels, num_points = feats
        pillars = self.reader(voxels, num_points, coors)
        pillars = pillars.reshape(-1, self.backbone.nchannels)      # the reader's .squeeze() drops the axis of a lone pillar
        return self.backbone(pillars, coors, batch_size, [int(grid[0]), int(grid[1])])
