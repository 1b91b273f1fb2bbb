"""Plain float64 reference of the one-layer PillarFeatureNet (efg/modeling/readers/pillar_encoder.py:98-132): the decoration,
the Linear and the max over the rows are written out here; the BatchNorm (+ ReLU) in between, its gradients and its running
statistics are `fp64_ref.batchnorm_fp64` over the P * N rows.  Nothing of efg_amd is imported.

Every value comes with the terms of the element-wise bar of `fp64_ref.assert_elementwise`,
|got - ref| <= c * sqrt(n) * 2^-24 * mag + cond:
  * a decorated feature is formed in fp32 from fp32 inputs: a cluster / centre column is a DIFFERENCE of two numbers that can
    both be ~70 m, so its magnitude is |x| + |mean or centre| (that subtraction is the formulation, not an error of the
    kernel); a raw column is exact (its magnitude still enters the products), the distance column has the magnitude of its
    value;
  * a pre-activation x[c] = sum_k W[c, k] f[k] has |terms| = sum_k |W[c, k]| mag_f[k], n = Cin;
  * behind the BatchNorm an error e of x arrives as rstd |gamma| e, next to the BatchNorm's own |terms| and its allowance
    `cond` for the rounded mean and rstd (fp64_ref.py, the normalisation section);
  * the max over the rows takes the largest bar of the rows: the value at ANY row within its bar of the maximum is a correct
    answer of an fp32 implementation;
  * the backward takes the forward's selected row as an ARGUMENT (`index`): the gradient enters there, gated by z > 0 in float64.
    dW[c, k] = sum over the rows of dx[m, c] f[m, k], with dx from batchnorm_fp64: |terms| = sum dx_mag mag_f (+ dx_cond |f|
    in cond), n = the real rows."""
import math

import torch

from fp64_ref import U32, assert_elementwise, batchnorm_fp64  # noqa: F401  (re-exported for the tests)

TIE_C = 16.0      # a selected pre-ReLU value within 16 x its bar of zero is a ReLU tie


def decorate_fp64(voxels, num_points, coors, vx, vy, x_offset, y_offset, with_distance):
    """-> (f, mag_f) float64 [P, N, Cin]: rows n >= num_points are zero whatever they hold.  vx, vy and the offsets are taken
    as the fp32 numbers the fp32 formulation multiplies and adds."""
    v = voxels.detach().to(torch.float64)
    p, n, _ = v.shape
    r32 = lambda s: float(torch.tensor(float(s), dtype=torch.float32))   # noqa: E731
    cnt = num_points.detach().to(torch.float64).view(p, 1, 1)
    xyz = v[:, :, :3]
    mean = xyz.sum(1, keepdim=True) / cnt                                   # over ALL rows, as the reference sums
    mean_mag = xyz.abs().sum(1, keepdim=True) / cnt
    cx = coors[:, 3].detach().to(torch.float64) * r32(vx) + r32(x_offset)
    cy = coors[:, 2].detach().to(torch.float64) * r32(vy) + r32(y_offset)
    centre = torch.stack([cx, cy], 1).view(p, 1, 2)
    cols = [v, xyz - mean, xyz[:, :, :2] - centre]
    mags = [v.abs(), xyz.abs() + mean_mag, xyz[:, :, :2].abs() + centre.abs()]
    if with_distance:
        dist = torch.sqrt((xyz ** 2).sum(2, keepdim=True))
        cols.append(dist)
        mags.append(dist)
    f, mag = torch.cat(cols, 2), torch.cat(mags, 2)
    real = (torch.arange(n, device=v.device).view(1, n) < num_points.view(p, 1)).unsqueeze(-1)
    zero = torch.zeros((), dtype=torch.float64, device=v.device)
    return torch.where(real, f, zero), torch.where(real, mag, zero)


def pillar_fp64(voxels, num_points, coors, weight, gamma, beta, running_mean, running_var, momentum, eps, vx, vy, x_offset,
                y_offset, with_distance, dy=None, index=None):
    """Training-mode forward (and, with dy [P, C] and index [P, C], the backward) of the layer in float64.

    Returns a dict.  Forward: out [P, C] with out_mag / out_n / out_cond; z [P, N, C] (pre-ReLU), y [P, N, C] and the per-row
    terms y_mag / y_cond; argmax [P, C] (lowest row of the float64 maximum); running_mean / running_var with _mag / _n /
    _cond; ties: the number of (p, c) whose float64-selected z lies within TIE_C x its bar of zero.
    Backward: dweight [C, Cin], dgamma, dbeta [C], each with _mag / _n / _cond."""
    f, mag_f = decorate_fp64(voxels, num_points, coors, vx, vy, x_offset, y_offset, with_distance)
    p, n, cin = f.shape
    w = weight.detach().to(torch.float64)
    c = w.shape[0]
    m = p * n
    x = (f @ w.t()).reshape(m, c)
    x_mag = (mag_f @ w.abs().t()).reshape(m, c)
    full_dy = None
    if dy is not None:
        full_dy = torch.zeros(p, n, c, dtype=torch.float64, device=f.device)
        full_dy.scatter_(1, index.long().view(p, 1, c), dy.detach().to(torch.float64).view(p, 1, c))
        full_dy = full_dy.reshape(m, c)
    bn = batchnorm_fp64(x, None, gamma, beta, running_mean, running_var, momentum, eps, True, full_dy)
    g64 = gamma.detach().to(torch.float64).view(1, c)
    mu = x.mean(0, keepdim=True)
    var = ((x - mu) ** 2).mean(0, keepdim=True)
    rstd = (var + eps) ** -0.5
    z = ((x - mu) * rstd * g64 + beta.detach().to(torch.float64).view(1, c)).view(p, n, c)
    y = bn["y"].view(p, n, c)
    carried = (x_mag * rstd * g64.abs()).view(p, n, c)            # the Linear's terms behind the BatchNorm
    y_mag = carried + bn["y_mag"].view(p, n, c)
    y_cond = bn["y_cond"].view(p, n, c)
    out = y.max(1).values
    first = (y == out.unsqueeze(1)).to(torch.int64).argmax(1)    # the lowest row at the maximum
    res = dict(out=out, out_mag=y_mag.max(1).values, out_n=cin, out_cond=y_cond.max(1).values, z=z, y=y, y_mag=y_mag,
               y_cond=y_cond, argmax=first, n_rows=m)
    z_sel = torch.gather(z, 1, first.view(p, 1, c)).view(p, c)
    bar_sel = (math.sqrt(cin) * U32 * torch.gather(y_mag, 1, first.view(p, 1, c)) + torch.gather(y_cond, 1, first.view(p, 1, c))).view(p, c)
    res["ties"] = int((z_sel.abs() <= TIE_C * bar_sel).sum())
    # running statistics: an error e of every x moves the mean by at most mean(e), the variance by 2 sqrt(var) rms(e)
    mom = float(momentum)
    unb = m / max(m - 1, 1)
    res.update(running_mean=bn["running_mean"], running_mean_n=max(m, cin), running_mean_cond=bn["running_mean_cond"],
               running_mean_mag=bn["running_mean_mag"] + mom * x_mag.mean(0),
               running_var=bn["running_var"], running_var_n=max(m, cin), running_var_cond=bn["running_var_cond"],
               running_var_mag=bn["running_var_mag"] + mom * unb * 2 * torch.sqrt(var.view(c)) * torch.sqrt((x_mag ** 2).mean(0)))
    if dy is None:
        return res
    dx, dx_mag, dx_cond = bn["dx"], bn["dx_mag"], bn["dx_cond"]
    f2, mag2 = f.reshape(m, cin), mag_f.reshape(m, cin)
    n_real = int(num_points.clamp(max=n).sum())
    gabs = (full_dy * (z.reshape(m, c) > 0)).abs()
    res.update(dweight=dx.t() @ f2, dweight_mag=dx_mag.t() @ mag2, dweight_n=max(n_real, 1), dweight_cond=dx_cond.t() @ f2.abs(),
               dgamma=bn["dweight"], dgamma_mag=bn["dweight_mag"] + (gabs * rstd * x_mag).sum(0), dgamma_n=m,
               dgamma_cond=bn["dweight_cond"],
               dbeta=bn["dbias"], dbeta_mag=bn["dbias_mag"], dbeta_n=m, dbeta_cond=bn["dbias_cond"])
    return res


def index_terms(index, ref):
    """(float64 value at the chosen row, float64 maximum, |terms|, cond) [P, C]: the two values may differ by the bars of both rows."""
    p, n, ch = ref["y"].shape
    at = index.long().view(p, 1, ch).to(ref["y"].device)
    assert int(at.max()) < n, "row %d of %d" % (int(at.max()), n)
    pick = lambda t: torch.gather(t, 1, at).view(p, ch)   # noqa: E731
    best = ref["argmax"].view(p, 1, ch)
    top = lambda t: torch.gather(t, 1, best).view(p, ch)  # noqa: E731
    return pick(ref["y"]), ref["out"], pick(ref["y_mag"]) + top(ref["y_mag"]), pick(ref["y_cond"]) + top(ref["y_cond"])


def check_index(name, index, ref, c):
    """The float64 value at the chosen row is within the bar of the float64 maximum."""
    value, best, mag, cond = index_terms(index, ref)
    return assert_elementwise(name, value, best, mag, ref["out_n"], c, geo64=cond)
