"""Plain float64 references for the sparse convolution, the fused box attention, the detection-loss tail (matching
cost, focal loss, box loss), scaled-dot-product attention with a boolean mask (forward, log-sum-exp and backward, written out from
the softmax) and the normalisation kernels (BatchNorm (+ residual) (+ ReLU) with its running statistics,
channels-last GroupNorm, residual-add + LayerNorm; written out from mean, biased variance and rstd, forward and backward),
and an element-wise error bar.

Nothing here imports efg_amd.spconv, the oracle or a HIP entry point: the rulebook is rebuilt from the int32 site
coordinates with torch.sort / searchsorted, the products are torch float64 matmuls, and the box-attention sampling is
written out from the bilinear formula.  The only project code used is `box_sampling_grid` (plain torch, pinned by the
model goldens), evaluated on float64 inputs.  Every function runs on the device of its inputs.

Error bar (`assert_elementwise`): an element that is a sum of n fp32 products must satisfy
|got - ref| <= c * sqrt(n) * 2^-24 * mag, where mag is the same sum taken over the absolute values of its terms.  The bar
is per ELEMENT: an element 1e-8 of its tensor's largest one is held to its own size, not to the largest one's.
"""
import math

import torch

U32 = 2.0 ** -24            # unit roundoff of float32
GEO_ULPS = 4                # coordinate shift allowed for the fp32 geometry, in units of 2^-23 x max(map side, |coordinate|)
_CHUNK_ELEMS = 1 << 27      # float64 elements per temporary: 1 GiB


# ---- error bar --------------------------------------------------------------------------------------------------------
def assert_elementwise(name, got, ref64, mag64, n_terms, c, geo64=None, tiny=1e-30):
    """Assert |got - ref64| <= c * sqrt(n_terms) * 2^-24 * mag64 (+ geo64) + tiny for EVERY element.

    `n_terms` is a number or a tensor broadcastable to `ref64` (terms per element).  `geo64` (optional) is an absolute
    allowance added as is: the box-attention reference passes the first-order change of each element when the sampling
    coordinates move by GEO_ULPS fp32 ulps (see `sample_fp64`).  Fails with the worst element's index and its err / bound
    ratio; returns the largest ratio."""
    assert c <= 16, "the rounding constant of a test is at most 16"
    got = got.detach().to(ref64.device, torch.float64)
    assert got.shape == ref64.shape, "%s: shape %s vs reference %s" % (name, tuple(got.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % name
    n = torch.as_tensor(n_terms, dtype=torch.float64, device=ref64.device).clamp_min(1.0)
    bound = c * torch.sqrt(n) * U32 * mag64 + tiny
    if geo64 is not None:
        bound = bound + geo64
    ratio = ((got - ref64).abs() / bound).reshape(-1)
    worst = int(torch.argmax(ratio))
    r = float(ratio[worst])
    if r > 1.0:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), tuple(ref64.shape)))
        raise AssertionError(
            "%s: %d of %d elements outside c=%g * sqrt(n) * 2^-24 * |terms|%s; worst at %s: got %.9g, ref %.9g, |terms| %.3g, "
            "err/bound %.3g" % (name, int((ratio > 1.0).sum()), ratio.numel(), c, " + geometry" if geo64 is not None else "",
                                idx, float(got[idx]), float(ref64[idx]), float(mag64[idx]), r))
    return r


# ---- sparse convolution -----------------------------------------------------------------------------------------------
def _keys(b, z, y, x, shape):
    d, h, w = shape
    return ((b.long() * d + z.long()) * h + y.long()) * w + x.long()


def independent_rulebook(indices, spatial_shape, ksize, stride, padding, subm):
    """Rulebook of a sparse 3-D convolution from int32 (b, z, y, x) rows.

    Returns (out_indices int32 [M, 4], out_shape [3], pairs) with pairs[k] = (in_rows, out_rows) int64 for the offset
    k = (kz * kh + ky) * kw + kx of a weight [Cout, kd, kh, kw, Cin].  Submanifold: the outputs are the input sites in input
    order, and output site o reads input site o + k - ksize // 2.  Strided: output o reads input o * stride - padding + k;
    the outputs are every such o inside the output grid that reads at least one input site, in ascending (b, z, y, x)
    order."""
    idx = indices.long()
    shape = [int(s) for s in spatial_shape]
    ks, st, pd = [int(v) for v in ksize], [int(v) for v in stride], [int(v) for v in padding]
    offsets = [(kz, ky, kx) for kz in range(ks[0]) for ky in range(ks[1]) for kx in range(ks[2])]
    if subm:
        in_sorted, in_perm = torch.sort(_keys(idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3], shape))
        pairs = []
        for k in offsets:
            p = [idx[:, 1 + a] + k[a] - ks[a] // 2 for a in range(3)]
            ok = torch.ones(len(idx), dtype=torch.bool, device=idx.device)
            for a in range(3):
                ok &= (p[a] >= 0) & (p[a] < shape[a])
            key = _keys(idx[:, 0], *p, shape)
            pos = torch.searchsorted(in_sorted, key).clamp_max(len(in_sorted) - 1)
            out_rows = torch.nonzero(ok & (in_sorted[pos] == key)).flatten()
            pairs.append((in_perm[pos[out_rows]], out_rows))
        return indices.clone(), shape, pairs
    out_shape = [(shape[a] + 2 * pd[a] - ks[a]) // st[a] + 1 for a in range(3)]
    cand = []
    for k in offsets:
        ok = torch.ones(len(idx), dtype=torch.bool, device=idx.device)
        o = []
        for a in range(3):
            q = idx[:, 1 + a] + pd[a] - k[a]
            oa = torch.div(q, st[a], rounding_mode="floor")
            ok &= (q >= 0) & (q - oa * st[a] == 0) & (oa < out_shape[a])
            o.append(oa)
        rows = torch.nonzero(ok).flatten()
        cand.append((rows, _keys(idx[rows, 0], *(oa[rows] for oa in o), out_shape)))
    out_keys = torch.unique(torch.cat([key for _, key in cand]))   # sorted ascending
    d, h, w = out_shape
    r = out_keys
    ox = r % w
    r = torch.div(r, w, rounding_mode="floor")
    oy = r % h
    r = torch.div(r, h, rounding_mode="floor")
    oz = r % d
    ob = torch.div(r, d, rounding_mode="floor")
    out_idx = torch.stack([ob, oz, oy, ox], 1).int()
    pairs = [(rows, torch.searchsorted(out_keys, key)) for rows, key in cand]
    return out_idx, out_shape, pairs


def spconv_fp64(x, w, go, pairs, m_out):
    """Forward, data gradient and weight gradient of a sparse convolution in float64, offset by offset (gather, matmul,
    index_add_), in chunks of at most ~1 GiB per temporary.

    x [m_in, Cin], w [Cout, kd, kh, kw, Cin] or [Cout, kvol, Cin], go [m_out, Cout] (or None: forward only).  Returns a dict:
    y [m_out, Cout], dx [m_in, Cin], dw [Cout, kvol, Cin]; y_mag, dx_mag, dw_mag: the same sums over |x|, |w| and |go|;
    n_y, n_dx, n_dw: the number of products in each element (active offsets x channels; pairs of the offset)."""
    dev = x.device
    cout, cin = w.shape[0], w.shape[-1]
    w3 = w.detach().reshape(cout, -1, cin).to(torch.float64)
    kvol = w3.shape[1]
    x64 = x.detach().to(torch.float64)
    xa, wa = x64.abs(), w3.abs()
    m_in = x64.shape[0]
    y = torch.zeros(m_out, cout, dtype=torch.float64, device=dev)
    y_mag = torch.zeros_like(y)
    k_out = torch.zeros(m_out, dtype=torch.float64, device=dev)
    if go is not None:
        g64 = go.detach().to(torch.float64)
        ga = g64.abs()
        dx = torch.zeros(m_in, cin, dtype=torch.float64, device=dev)
        dx_mag = torch.zeros_like(dx)
        k_in = torch.zeros(m_in, dtype=torch.float64, device=dev)
        dw = torch.zeros(cout, kvol, cin, dtype=torch.float64, device=dev)
        dw_mag = torch.zeros_like(dw)
        n_dw = torch.zeros(1, kvol, 1, dtype=torch.float64, device=dev)
    step = max(1, _CHUNK_ELEMS // max(cin, cout))
    for k, (in_rows, out_rows) in enumerate(pairs):
        wk, wak = w3[:, k, :], wa[:, k, :]
        k_out.index_add_(0, out_rows, torch.ones(len(out_rows), dtype=torch.float64, device=dev))
        if go is not None:
            k_in.index_add_(0, in_rows, torch.ones(len(in_rows), dtype=torch.float64, device=dev))
            n_dw[0, k, 0] = len(in_rows)
        for s in range(0, len(in_rows), step):
            ir, orow = in_rows[s:s + step], out_rows[s:s + step]
            xi, xai = x64[ir], xa[ir]
            y.index_add_(0, orow, xi @ wk.t())
            y_mag.index_add_(0, orow, xai @ wak.t())
            if go is not None:
                gi, gai = g64[orow], ga[orow]
                dx.index_add_(0, ir, gi @ wk)
                dx_mag.index_add_(0, ir, gai @ wak)
                dw[:, k, :] += gi.t() @ xi
                dw_mag[:, k, :] += gai.t() @ xai
    res = dict(y=y, y_mag=y_mag, n_y=(k_out * cin).unsqueeze(1))
    if go is not None:
        res.update(dx=dx, dx_mag=dx_mag, n_dx=(k_in * cout).unsqueeze(1), dw=dw, dw_mag=dw_mag, n_dw=n_dw)
    return res


# ---- box attention ----------------------------------------------------------------------------------------------------
def _corners(px, py):
    """The 4 bilinear corners of pixel coordinates (px, py): (x, y, weight, d weight / d px, d weight / d py) each."""
    x0, y0 = torch.floor(px), torch.floor(py)
    fx, fy = px - x0, py - y0
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            wx, dwx = (fx, 1.0) if dx else (1 - fx, -1.0)
            wy, dwy = (fy, 1.0) if dy else (1 - fy, -1.0)
            out.append((x0 + dx, y0 + dy, wx * wy, dwx * wy, wx * dwy))
    return out


def sample_fp64(value, shapes, starts, loc, attn, grad_out=None, geo_ulps=GEO_ULPS, reference_inside=False):
    """Multi-scale bilinear sampling (the sampling op of box / deformable attention) in float64, written out by hand.

    value [B, S, H, D], shapes [L, 2] (h, w), starts [L], loc [B, Q, H, L, P, 2] normalised (x, y), attn [B, Q, H, L, P],
    grad_out [B, Q, H * D] or None.  Convention of grid_sample(align_corners=False, padding_mode="zeros"): pixel =
    normalised * side - 0.5, corners outside the map read zero.

    Returns out [B, Q, H * D] and, with grad_out, grad_value [B, S, H, D], grad_loc, grad_attn; for each `<name>_mag` (the
    same sum over absolute values: |value|, |grad_out|, the bilinear and attention weights and |d weight / d pixel|) and
    `<name>_geo`, the allowance for the kernels' fp32 geometry: the first-order change of the element when every pixel
    coordinate moves by GEO_ULPS x 2^-23 x max(map side, |coordinate|) -- a few fp32 ulps of a coordinate of the size of
    the map -- in whichever direction hurts, computed in fp64.  It is first order only: with no sampling point within
    1e-3 px of a cell boundary both sides interpolate between the same four corners.  The bilinear weight is linear in each
    coordinate, so the geometry term of grad_loc is the mixed second derivative (|d2 w / dpx dpy| = 1).  grad_value_n:
    the number of (point, corner) entries summed into each grad_value row.

    `reference_inside` (default off) applies the rule of the kernels and of the CUDA reference (box_attn_kernel.cuh) to the
    WHOLE point: a point takes part only if px > -1 && py > -1 && px < W && py < H.  It differs from the per-corner rule
    only at px == -1 or py == -1 exactly, where the one corner in range has weight 0 but a one-sided derivative of the
    weight that is not 0: with the keyword such a point contributes nothing, grad_loc included."""
    b, s, h, d = value.shape
    q, nl, p = loc.shape[1], loc.shape[3], loc.shape[4]
    dev = value.device
    vflat = value.to(torch.float64).permute(0, 2, 1, 3).reshape(b * h * s, d)   # row (b, h, cell)
    vabs = vflat.abs()
    a = attn.to(torch.float64)
    base = ((torch.arange(b, device=dev).view(b, 1, 1, 1) * h + torch.arange(h, device=dev).view(1, 1, h, 1)) * s)
    out = torch.zeros(b, q, h, d, dtype=torch.float64, device=dev)
    out_mag, out_geo = torch.zeros_like(out), torch.zeros_like(out)
    with_grad = grad_out is not None
    if with_grad:
        g = grad_out.to(torch.float64).reshape(b, q, h, 1, d)
        gabs = g.abs()
        gv, gv_mag, gv_geo = torch.zeros_like(vflat), torch.zeros_like(vflat), torch.zeros_like(vflat)
        gv_n = torch.zeros(b * h * s, 1, dtype=torch.float64, device=dev)
        gl = torch.zeros(b, q, h, nl, p, 2, dtype=torch.float64, device=dev)
        gl_mag, gl_geo = torch.zeros_like(gl), torch.zeros_like(gl)
        ga = torch.zeros(b, q, h, nl, p, dtype=torch.float64, device=dev)
        ga_mag, ga_geo = torch.zeros_like(ga), torch.zeros_like(ga)
    for lv in range(nl):
        hl, wl, st = int(shapes[lv, 0]), int(shapes[lv, 1]), int(starts[lv])
        px = loc[:, :, :, lv, :, 0].to(torch.float64) * wl - 0.5          # [B, Q, H, P]
        py = loc[:, :, :, lv, :, 1].to(torch.float64) * hl - 0.5
        dpx = geo_ulps * 2.0 ** -23 * torch.clamp(px.abs(), min=float(wl))
        dpy = geo_ulps * 2.0 ** -23 * torch.clamp(py.abs(), min=float(hl))
        al = a[:, :, :, lv, :]
        if reference_inside:
            whole = ((px > -1) & (py > -1) & (px < wl) & (py < hl)).to(torch.float64)
        for cx, cy, wgt, dwx, dwy in _corners(px, py):
            inside = ((cx >= 0) & (cx < wl) & (cy >= 0) & (cy < hl)).to(torch.float64)
            if reference_inside:
                inside = inside * whole
            row = base + st + (cy.clamp(0, hl - 1) * wl + cx.clamp(0, wl - 1)).long()   # [B, Q, H, P]
            vc = vflat[row] * inside.unsqueeze(-1)                                      # [B, Q, H, P, D]
            vca = vc.abs()
            aw = al * wgt * inside
            shift = (dwx.abs() * dpx + dwy.abs() * dpy) * inside    # first-order change of the weight
            out += (aw.unsqueeze(-1) * vc).sum(3)
            out_mag += (aw.unsqueeze(-1) * vca).sum(3)
            out_geo += ((al * shift).unsqueeze(-1) * vca).sum(3)
            if with_grad:
                dot = (vc * g).sum(-1)                                                  # [B, Q, H, P]
                adot = (vca * gabs).sum(-1)
                ga[:, :, :, lv] += wgt * dot
                ga_mag[:, :, :, lv] += wgt * adot
                ga_geo[:, :, :, lv] += shift * adot
                gl[:, :, :, lv, :, 0] += al * dwx * dot * wl
                gl[:, :, :, lv, :, 1] += al * dwy * dot * hl
                gl_mag[:, :, :, lv, :, 0] += al * dwx.abs() * adot * wl
                gl_mag[:, :, :, lv, :, 1] += al * dwy.abs() * adot * hl
                gl_geo[:, :, :, lv, :, 0] += al * adot * dpy * wl
                gl_geo[:, :, :, lv, :, 1] += al * adot * dpx * hl
                rflat = row.reshape(-1)
                gv.index_add_(0, rflat, (aw.unsqueeze(-1) * g).reshape(-1, d))
                gv_mag.index_add_(0, rflat, (aw.unsqueeze(-1) * gabs).reshape(-1, d))
                gv_geo.index_add_(0, rflat, ((al * shift).unsqueeze(-1) * gabs).reshape(-1, d))
                gv_n.index_add_(0, rflat, inside.reshape(-1, 1))
    res = dict(out=out.reshape(b, q, h * d), out_mag=out_mag.reshape(b, q, h * d), out_geo=out_geo.reshape(b, q, h * d))
    if with_grad:
        unflat = lambda t: t.reshape(b, h, s, t.shape[-1]).permute(0, 2, 1, 3)   # noqa: E731
        res.update(grad_value=unflat(gv), grad_value_mag=unflat(gv_mag), grad_value_geo=unflat(gv_geo),
                   grad_value_n=unflat(gv_n), grad_loc=gl, grad_loc_mag=gl_mag, grad_loc_geo=gl_geo,
                   grad_attn=ga, grad_attn_mag=ga_mag, grad_attn_geo=ga_geo)
    return res


def box_attention_fp64(value, shapes, starts, ref, offsets, logits, kidx, num_var, grad_out, chunk=1024):
    """The fused box-attention op -- box geometry, softmax over the L * P logits of a (query, head), bilinear sampling --
    and its gradients in float64.

    value [B, S, H, D], shapes [L, 2], starts [L], ref [B, Q, 7], offsets [B, Q, H * L * num_var], logits [B, Q, H * L * P],
    kidx [P, 2], grad_out [B, Q, H * D].  The geometry is `box_sampling_grid` on float64 inputs, the sampling is
    `sample_fp64`, autograd carries its grad_loc / grad_attn back through the geometry and the softmax.  `chunk` queries
    at a time.  Returns out, grad_value, grad_offsets, grad_logits, each with `_mag`, `_geo` (see `sample_fp64`; carried
    back through |d grid / d offset| and the softmax) and `_n` (products per element); px, py [B, Q, H, L, P]: the
    float64 pixel coordinates of every sampling point."""
    from efg_amd.operators.box_attention_func import box_sampling_grid

    b, s, h, d = value.shape
    q, nl, p = ref.shape[1], shapes.shape[0], kidx.shape[0]
    rot = num_var == 5
    dev = value.device
    v64 = value.detach().to(torch.float64)
    k64 = kidx.detach().to(torch.float64)
    r64 = ref.detach().to(torch.float64)
    shapes_h, starts_h = shapes.cpu(), starts.cpu()
    side_w = torch.tensor([float(shapes_h[lv, 1]) for lv in range(nl)], dtype=torch.float64, device=dev).view(1, 1, 1, nl, 1)
    side_h = torch.tensor([float(shapes_h[lv, 0]) for lv in range(nl)], dtype=torch.float64, device=dev).view(1, 1, 1, nl, 1)
    parts = {k: [] for k in ("out", "out_mag", "out_geo", "grad_offsets", "grad_offsets_mag", "grad_offsets_geo",
                             "grad_logits", "grad_logits_mag", "grad_logits_geo", "px", "py")}
    gv = None
    for q0 in range(0, q, chunk):
        q1 = min(q, q0 + chunk)
        n = q1 - q0
        rc = r64[:, q0:q1]
        off = offsets[:, q0:q1].detach().to(torch.float64).requires_grad_(True)
        lg = logits[:, q0:q1].detach().to(torch.float64).requires_grad_(True)
        grid = box_sampling_grid(rc, off, k64, h, nl, rot)                                   # [B, n, H, L, P, 2]
        attn = torch.softmax(lg.view(b, n, h, nl * p), dim=-1).view(b, n, h, nl, p)
        smp = sample_fp64(v64, shapes_h, starts_h, grid.detach(), attn.detach(), grad_out[:, q0:q1])
        torch.autograd.backward([grid, attn], [smp["grad_loc"], smp["grad_attn"]])
        # behind the softmax: d logit_i = a_i (g_i - sum_j a_j g_j)  ->  a_i (|g_i| + sum_j a_j |g_j|)
        av = attn.detach().view(b, n, h, nl * p)
        for t in ("mag", "geo"):
            gt = smp["grad_attn_" + t].view(b, n, h, nl * p)
            parts["grad_logits_" + t].append((av * (gt + (av * gt).sum(-1, keepdim=True))).reshape(b, n, -1))
        # behind the geometry: sum over the points of |d grid / d offset_j| x the point's bound (forward mode, one j at a time)
        om, og = torch.zeros_like(off), torch.zeros_like(off)
        for j in range(num_var):
            tan = torch.zeros(b, n, h, nl, num_var, dtype=torch.float64, device=dev)
            tan[..., j] = 1
            _, jac = torch.func.jvp(lambda o: box_sampling_grid(rc, o, k64, h, nl, rot), (off.detach(),),
                                    (tan.reshape(off.shape),))
            jac = jac.abs()
            om.view(b, n, h, nl, num_var)[..., j] = (jac * smp["grad_loc_mag"]).sum((-1, -2))
            og.view(b, n, h, nl, num_var)[..., j] = (jac * smp["grad_loc_geo"]).sum((-1, -2))
        parts["grad_offsets"].append(off.grad)
        parts["grad_offsets_mag"].append(om)
        parts["grad_offsets_geo"].append(og)
        parts["grad_logits"].append(lg.grad)
        for k in ("out", "out_mag", "out_geo"):
            parts[k].append(smp[k])
        gd = grid.detach()
        parts["px"].append(gd[..., 0] * side_w - 0.5)
        parts["py"].append(gd[..., 1] * side_h - 0.5)
        if gv is None:
            gv = {t: smp["grad_value" + t] for t in ("", "_mag", "_geo", "_n")}
        else:
            for t in gv:
                gv[t] += smp["grad_value" + t]
        del smp, grid, attn
    res = {k: torch.cat(v, 1) for k, v in parts.items()}
    res.update({"grad_value" + t: v for t, v in gv.items()})
    # products per element: 4 corners x L x P points (out); D channels x 4 corners x L x P points (logits, offsets)
    res["out_n"] = 4 * nl * p
    res["grad_logits_n"] = res["grad_offsets_n"] = 4 * nl * p * d
    return res


def binned_sum_allowance(n_entries, grad_out):
    """Resolution of the fused backward's binned grad_value sums (box_bin_reduce_kernel): each product w * g is
    rounded to an integer multiple of 2^-sh, sh = min(50, 62 - ln) - ex, where n + 1 <= 2^ln and 2^ex bounds
    2 * max |grad_out| of the call, so a row of n entries is exact to n * 2^-(sh+1) in absolute terms (~1e-13 of the largest
    |grad_out| per entry).  `n_entries` counts every corner of the row -- at least the binned ones -- so this is an upper
    bound."""
    import numpy as np

    gmax = np.float32(grad_out.detach().abs().max().cpu())
    ex = math.frexp(float(min(gmax * np.float32(2.0000002), np.float32(3.0e38))))[1]
    n = n_entries.to(torch.float64)
    sh = torch.clamp(62 - torch.ceil(torch.log2(n + 1)), max=50) - ex
    return n * torch.pow(2.0, -(sh + 1))


def near_cell_boundary(px, py, tol=1e-3):
    """Sampling points whose pixel coordinate lies within `tol` px of an integer (a boundary of the bilinear cells)."""
    fx, fy = px - torch.floor(px), py - torch.floor(py)
    return (torch.minimum(fx, 1 - fx) < tol) | (torch.minimum(fy, 1 - fy) < tol)


def log_uniform_signed(shape, lo, hi, gen):
    """float32 values with magnitudes log-uniform in [lo, hi] and random signs (CPU generator)."""
    mag = torch.exp(torch.empty(shape, dtype=torch.float64).uniform_(math.log(lo), math.log(hi), generator=gen))
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0).to(torch.float64)
    return (mag * sign).float()


# ---- detection losses: matching cost, focal loss, box loss (csrc/det_loss.hip) -----------------------------------------
# Written out from the definitions ($CQ/modules/matcher.py:40-80, $CQ/losses.py:26-108, efg/modeling/losses/focal_loss.py);
# nothing of efg_amd is imported.  Next to every value come `<name>_mag` (the same expression over the absolute values of
# its terms), `<name>_n` (terms per element) and `<name>_cond`, an ABSOLUTE allowance for assert_elementwise's `geo64`: these
# formulas are ill-conditioned by construction (1 - p for p near 1, log(1 - p + 1e-8), corners c +- s/2 of a thin box far
# from the origin), and ANY fp32 evaluation from the fixed fp32 inputs rounds these intermediates.  `cond` is the first-order
# effect, in float64, of a relative change of 2^-24 in each of them, in whichever direction hurts: sum_v |v * d out / d v|
# * 2^-24 over the rounded values v that make up p = sigmoid(x) = 1 / (1 + exp(-x)) -- exp(-x), 1 + exp(-x) and the reciprocal:
# an fp32 sigmoid is three rounded operations, and for p near 1 it is 1.4 x 2^-24 off in torch and in 1 / (1 + expf(-x)) alike
# --; v = 1 - p; v = p + 1e-8 and 1 - p + 1e-8 (matching cost only); the twelve box corners.  Every v carries a multiplicative
# leaf (1 + e_v), e_v = 0, and autograd returns d out / d e_v = v * d out / d v with everything computed from v following it.
# `cond` never sees a kernel's output.
def _zeros_leaf(like):
    return torch.zeros_like(like, dtype=torch.float64).requires_grad_(True)


def _sigmoid_rounded(x):
    """sigmoid(x) as 1 / (1 + exp(-x)) with a leaf on each of its three rounded values; returns p and the leaves."""
    e = [_zeros_leaf(x) for _ in range(3)]
    return (1 + e[2]) / ((1 + torch.exp(-x) * (1 + e[0])) * (1 + e[1])), e


def _sensitivity(out, leaves):
    """sum over the leaves e of |d out[i] / d e[i, ...]| * 2^-24 for an `out` each of whose elements depends only on the
    leaves' elements of the same leading index (leaves may carry trailing axes)."""
    grads = torch.autograd.grad(out.sum(), leaves, retain_graph=True, allow_unused=True)
    total = torch.zeros_like(out)
    for g in grads:
        if g is not None:
            a = g.detach().abs()
            total = total + (a.reshape(*out.shape, -1).sum(-1) if a.dim() > out.dim() else a)
    return total * U32


def _box_corners(box):
    """(lo, hi) [..., 3] of (centre, size) boxes [..., >= 6]."""
    return box[..., :3] - 0.5 * box[..., 3:6], box[..., :3] + 0.5 * box[..., 3:6]


def _giou_parts(vols, inters, encl):
    """Axis-aligned 3-D IoU and the enclosing-box term of GIoU = iou - (vol - union) / vol, from corner sets (slo, shi, tlo,
    thi): the two volumes from `vols`, the intersection from `inters`, the enclosing box from `encl` (the same set three
    times, or three copies that let a caller tell the three paths of a gradient apart).  Returns iou, (vol - union) / vol,
    (vol + union) / vol."""
    slo, shi, tlo, thi = vols
    v1, v2 = (shi - slo).prod(-1), (thi - tlo).prod(-1)
    slo, shi, tlo, thi = inters
    inter = (torch.minimum(shi, thi) - torch.maximum(slo, tlo)).clamp(min=0).prod(-1)
    union = v1 + v2 - inter
    slo, shi, tlo, thi = encl
    vol = (torch.maximum(shi, thi) - torch.minimum(slo, tlo)).clamp(min=0).prod(-1)
    return inter / union, (vol - union) / vol, (vol + union) / vol


def match_cost_fp64(logits, boxes, tgt_labels, tgt_boxes, w_class, w_bbox, w_giou, w_rad, alpha=0.25, gamma=2.0):
    """The matching cost of every (layer, scene, query, target column) in float64.

    logits [L, B, Q, C], boxes [L, B, Q, 7], tgt_labels [B, G] int64, tgt_boxes [B, G, 7].  cost = w_bbox * L1(centre, size) +
    w_class * (pos - neg) + w_giou * (-GIoU) + w_rad * |d angle|, with p = sigmoid(logit of the column's class), pos =
    alpha (1 - p)^gamma (-log(p + 1e-8)), neg = (1 - alpha) p^gamma (-log(1 - p + 1e-8)).  Returns a dict: cost [L * B, Q, G],
    cost_mag (the L1 terms, pos + neg, iou + (vol + union) / vol, under |weights|), cost_n (1) and cost_cond (see above)."""
    nl, b, q, _ = logits.shape
    g = tgt_labels.shape[1]
    lab = tgt_labels.long()[None, :, None, :].expand(nl, b, q, g)
    x = torch.gather(logits.detach().to(torch.float64), 3, lab)                      # [L, B, Q, G]
    bx = boxes.detach().to(torch.float64)[:, :, :, None, :].expand(nl, b, q, g, 7)
    tb = tgt_boxes.detach().to(torch.float64)[None, :, None, :, :].expand(nl, b, q, g, 7)
    e_q, e_a, e_b = (_zeros_leaf(x) for _ in range(3))
    p, e_p = _sigmoid_rounded(x)
    one_m = (1 - p) * (1 + e_q)
    la, lb = -torch.log((p + 1e-8) * (1 + e_a)), -torch.log((one_m + 1e-8) * (1 + e_b))
    pos, neg = alpha * one_m ** gamma * la, (1 - alpha) * p ** gamma * lb
    e_c = [_zeros_leaf(bx[..., :3]) for _ in range(4)]
    corners = [c * (1 + e) for c, e in zip(_box_corners(bx) + _box_corners(tb), e_c)]
    iou, enc, enc_mag = _giou_parts(corners, corners, corners)
    l1 = (bx[..., :6] - tb[..., :6]).abs().sum(-1)
    rad = (bx[..., 6] - tb[..., 6]).abs()
    cost = w_bbox * l1 + w_class * (pos - neg) + w_giou * -(iou - enc) + w_rad * rad
    mag = abs(w_bbox) * l1 + abs(w_class) * (pos.abs() + neg.abs()) + abs(w_giou) * (iou + enc_mag) + abs(w_rad) * rad
    cond = _sensitivity(cost, e_p + [e_q, e_a, e_b] + e_c)
    shape = (nl * b, q, g)
    return dict(cost=cost.detach().reshape(shape), cost_mag=mag.detach().reshape(shape), cost_n=1,
                cost_cond=cond.reshape(shape))


def focal_terms(x, hit, alpha, gamma, p, one_m_p):
    """The focal loss element and its derivative to the logit as formulas of x, p and the rounded 1 - p: ce = max(x, 0) - x t
    + log1p(exp(-|x|)), p_t = p t + (1 - p)(1 - t), loss = a_t ce (1 - p_t)^gamma; d ce / dx = p - t, d p_t / dx = +- p (1 - p).
    Returns loss, the two terms of the derivative."""
    t = hit.to(x.dtype)
    ce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    one_m = torch.where(hit, one_m_p, 1 - one_m_p)          # 1 - p_t
    a_t = (alpha * t + (1 - alpha) * (1 - t)) if alpha >= 0 else torch.ones_like(t)
    dpt = torch.where(hit, 1.0, -1.0) * p * one_m_p
    return a_t * ce * one_m ** gamma, a_t * (p - t) * one_m ** gamma, -a_t * ce * gamma * one_m ** (gamma - 1) * dpt


def focal_fp64(logits, tcls, denom, alpha, gamma, grad_out):
    """Per-layer sums of the sigmoid focal loss against class-index targets (-1: background) and their gradient, float64.

    logits [L, ..., C], tcls int [L, ...], grad_out [L].  Returns loss [L] = sum / denom with loss_mag (= loss: every element
    is non-negative), loss_n (elements per layer), loss_cond; grad [as logits] from float64 autograd through the definition,
    grad_mag (|its two terms|), grad_n (1), grad_cond."""
    nl, c = logits.shape[0], logits.shape[-1]
    x = logits.detach().to(torch.float64).reshape(nl, -1, c)
    hit = tcls.reshape(nl, -1, 1).long() == torch.arange(c, device=x.device).view(1, 1, c)
    go = grad_out.detach().to(torch.float64).reshape(nl, 1, 1) / float(denom)
    xl = x.clone().requires_grad_(True)
    pl = torch.sigmoid(xl)
    loss = focal_terms(xl, hit, alpha, gamma, pl, 1 - pl)[0]
    grad, = torch.autograd.grad((loss * go).sum(), xl)
    e_q = _zeros_leaf(x)
    p, e_p = _sigmoid_rounded(x)
    val, g1, g2 = focal_terms(x, hit, alpha, gamma, p, (1 - p) * (1 + e_q))
    per_layer = loss.detach().sum((1, 2)) / float(denom)
    return dict(loss=per_layer, loss_mag=per_layer.clone(), loss_n=x.shape[1] * c,
                loss_cond=_sensitivity(val, e_p + [e_q]).sum((1, 2)) / abs(float(denom)),
                grad=grad.reshape(logits.shape), grad_mag=((g1.abs() + g2.abs()).detach() * go.abs()).reshape(logits.shape),
                grad_n=1, grad_cond=(_sensitivity(g1 + g2, e_p + [e_q]) * go.abs()).reshape(logits.shape),
                grad_formula=((g1 + g2).detach() * go).reshape(logits.shape))


def box_loss_fp64(boxes, tgt_boxes, l_idx, b_idx, q_idx, g_idx, denom, grad_out):
    """Per-layer sums of (L1 of centre and size, 1 - GIoU, |d angle|) over matched (prediction, target) pairs, and the
    gradient to the predicted boxes, in float64.

    boxes [L, B, Q, 7], tgt_boxes [B, G, 7], pair i = prediction (l, b, q)[i] against target (b, g)[i]; pairs with q < 0 or
    q >= Q are skipped; a (l, b, q) row occurs at most once.  grad_out [L, 3].  The gradient is float64 autograd through
    abs, minimum / maximum and clamp(min=0), so every tie is autograd's choice: half each at equal corners, the clamp passes at
    exactly 0, sign(0) = 0.  Returns loss [L, 3] with loss_mag (= loss, the elements are non-negative), loss_n [L, 3] (summed
    elements: 6 / 1 / 1 per pair), loss_cond; grad [L, B, Q, 7] (zero in unmatched rows) with grad_mag (the L1 sign plus, for
    GIoU, |the gradient through the two volumes| + |through the intersection| + |through the enclosing box| at each
    corner), grad_n (1), grad_cond; rows [L, B, Q] bool: the matched rows."""
    nl, nb, nq = boxes.shape[:3]
    dev = boxes.device
    ok = (q_idx >= 0) & (q_idx < nq)
    li, bi, qi, gi = (t[ok].long() for t in (l_idx, b_idx, q_idx, g_idx))
    n = li.numel()
    src = boxes.detach().to(torch.float64)[li, bi, qi]                                 # [n, 7]
    tgt = tgt_boxes.detach().to(torch.float64)[bi, gi]
    w = grad_out.detach().to(torch.float64)[li] / float(denom)                        # [n, 3]

    def per_pair(s, sets):
        iou, enc, _ = _giou_parts(*sets)
        return torch.stack(((s[:, :6] - tgt[:, :6]).abs().sum(1), 1 - (iou - enc), (s[:, 6] - tgt[:, 6]).abs()), dim=1)

    sl = src.clone().requires_grad_(True)
    cs = list(_box_corners(sl) + _box_corners(tgt))
    per = per_pair(sl, (cs, cs, cs))
    gsrc, = torch.autograd.grad((per * w).sum(), sl) if n else (torch.zeros_like(src),)
    loss = torch.zeros(nl, 3, dtype=torch.float64, device=dev).index_add_(0, li, per.detach()) / float(denom)
    count = torch.zeros(nl, dtype=torch.float64, device=dev).index_add_(0, li, torch.ones(n, dtype=torch.float64, device=dev))

    # conditioning and magnitudes: corners c (1 + e); the three paths of the GIoU gradient read their own additive copies
    e_c = [_zeros_leaf(src[:, :3]) for _ in range(4)]
    base = [c * (1 + e) for c, e in zip(_box_corners(src) + _box_corners(tgt), e_c)]
    z = [[_zeros_leaf(src[:, :3]) for _ in range(2)] for _ in range(3)]                # path x (lo, hi) of the prediction
    sets = [[base[0] + zp[0], base[1] + zp[1], base[2], base[3]] for zp in z]
    iou, enc, _ = _giou_parts(*sets)
    gl = 1 - (iou - enc)
    cond_pair = _sensitivity(gl, e_c) if n else gl.detach()
    loss_cond = torch.zeros(nl, 3, dtype=torch.float64, device=dev)
    loss_cond[:, 1] = torch.zeros(nl, dtype=torch.float64, device=dev).index_add_(0, li, cond_pair) / abs(float(denom))
    g_mag, g_cond = torch.zeros_like(src), torch.zeros_like(src)
    if n:
        flat = torch.autograd.grad((gl * w[:, 1]).sum(), [t for zp in z for t in zp], create_graph=True)
        g_lo, g_hi = flat[0] + flat[2] + flat[4], flat[1] + flat[3] + flat[5]
        m_lo = sum(flat[i].detach().abs() for i in (0, 2, 4))
        m_hi = sum(flat[i].detach().abs() for i in (1, 3, 5))
        sgn_mag = (src - tgt).sign().abs()
        g_mag[:, :3] = w[:, :1].abs() * sgn_mag[:, :3] + m_hi + m_lo
        g_mag[:, 3:6] = w[:, :1].abs() * sgn_mag[:, 3:6] + 0.5 * (m_hi + m_lo)
        g_mag[:, 6] = w[:, 2].abs() * sgn_mag[:, 6]
        for k in range(3):
            g_cond[:, k] = _sensitivity((g_hi + g_lo)[:, k], e_c)
            g_cond[:, 3 + k] = _sensitivity(0.5 * (g_hi - g_lo)[:, k], e_c)

    def rows_of(v):
        out = torch.zeros(nl, nb, nq, 7, dtype=torch.float64, device=dev)
        out[li, bi, qi] = v
        return out

    rows = torch.zeros(nl, nb, nq, dtype=torch.bool, device=dev)
    rows[li, bi, qi] = True
    return dict(loss=loss, loss_mag=loss.clone(), loss_n=count.view(nl, 1) * torch.tensor([6.0, 1.0, 1.0], dtype=torch.float64, device=dev),
                loss_cond=loss_cond, grad=rows_of(gsrc), grad_mag=rows_of(g_mag), grad_n=1, grad_cond=rows_of(g_cond), rows=rows)


# ---- normalisation: BatchNorm (+ residual) (+ ReLU), GroupNorm, residual-add + LayerNorm (csrc/batchnorm.hip, layernorm.hip) --
# One operation with three reduction sets, written out: mu = mean(x), var = mean((x - mu)^2) (biased), rstd = (var + eps)^-1/2,
# xhat = (x - mu) rstd, y = relu?(xhat w + b + residual); backward, with dy' = dy [y > 0] and g = w dy':
#   dx = rstd (g - mean(g) - xhat mean(g xhat)),  d residual = dy',  dw = sum dy' xhat,  db = sum dy'
# (means over the statistics set of the element, sums over everything that shares the parameter).  Nothing of efg_amd and no
# torch *_norm is used.  `_mag` is the same expression over absolute values, `_n` the number of terms summed into the element
# (1 for y; the size of the statistics set for dx; the rows of a parameter for dw / db).  `_cond` is an ABSOLUTE allowance for
# assert_elementwise's `geo64`: any fp32 evaluation rounds the two statistics, the mean by about sqrt(n) 2^-24 mean|x| (a sum of
# n values) and rstd by a relative (sqrt(n) + 2) 2^-24 (the variance is a sum of n non-negative terms; + 2 for the square root
# and the divide), and on top of that takes the variance about its ROUNDED mean, sum (x - mu')^2 = sum (x - mu)^2 + n (mu' - mu)^2,
# which moves rstd by another relative d_mu^2 / (2 (var + eps)) -- second order, and the only term that matters when the data sit
# far from 0 (x = 1000 +- 0.01).  `_cond` = |d out / d mu| d_mu + |d out / d rstd| d_rstd, taken in float64 with torch.func.jvp
# of the written-out formula; one tangent holds all statistics at once because every element depends on exactly one of each
# kind.  The Taylor terms of second order (1/2 |d2 / d mu2| d_mu^2 + |d2 / d mu d rstd| d_mu d_rstd + 1/2 |d2 / d rstd2| d_rstd^2,
# nested jvp) are added: with x = 1000 +- 0.01 in a set of four, rstd d_mu reaches 1e-2, and where the first-order term of an
# element happens to vanish the second-order one is still 1e-4 of the element, a hundred times the rounding bar.  For dw (db does not see the statistics) it is the sum of the per-term absolute sensitivities.  With it a constant
# channel (var = 0, rstd = eps^-1/2) and a large offset are well-defined cases: the reference is 0 where fp32 is not.  It never
# sees a kernel's output.
# ReLU ties: an element whose float64 pre-activation lies within its own forward bound (at the cap c = NORM_TIE_C) of 0 may
# take either side of y > 0.  `near_zero` marks them; dx and d residual of those elements are not compared, and what a flip
# moves elsewhere -- sum_near_zero |dy| in db, |dy xhat| in dw, and the two means inside dx -- is added to `_cond`.
NORM_TIE_C = 16.0


def _norm_fp64(x, stat_dims, par_dims, w, b, res, eps, relu, dy):
    """The core: x float64 of any rank, statistics over `stat_dims`, w and b broadcastable to x and constant over `par_dims`,
    res like x or None, dy like x or None.  Returns a dict of float64 tensors (statistics with keepdim, dweight / dbias with
    keepdim over par_dims)."""
    n = 1
    for d in stat_dims:
        n *= x.shape[d]
    n = max(n, 1)
    mu = x.mean(stat_dims, keepdim=True)
    var = ((x - mu) ** 2).mean(stat_dims, keepdim=True)
    rstd = (var + eps) ** -0.5
    d_mu = math.sqrt(n) * U32 * x.abs().mean(stat_dims, keepdim=True)
    d_rs = rstd * ((math.sqrt(n) + 2) * U32 + 0.5 * d_mu ** 2 / (var + eps))
    r0 = res if res is not None else torch.zeros((), dtype=x.dtype, device=x.device)

    def sens(f):
        """[|d out / d mu| d_mu + |d out / d rstd| d_rstd, carried to second order, for each output of f(mu, rstd)]"""
        zm, zs = torch.zeros_like(mu), torch.zeros_like(rstd)
        t_mu, t_rs = (d_mu, zs), (zm, d_rs)
        along = lambda t: (lambda m, s: torch.func.jvp(f, (m, s), t)[1])   # noqa: E731
        j_m, j_mm = torch.func.jvp(along(t_mu), (mu, rstd), t_mu)
        j_s, j_ss = torch.func.jvp(along(t_rs), (mu, rstd), t_rs)
        _, j_ms = torch.func.jvp(along(t_mu), (mu, rstd), t_rs)
        return [a.abs() + b.abs() + 0.5 * aa.abs() + ab.abs() + 0.5 * bb.abs() for a, b, aa, ab, bb in zip(j_m, j_s, j_mm, j_ms, j_ss)]

    def fwd(m, s):
        return ((x - m) * s * w + b + r0,)

    pre, = fwd(mu, rstd)
    y_mag = (x - mu).abs() * rstd * w.abs() + b.abs() + r0.abs()
    y_cond, = sens(fwd)
    out = dict(mean=mu, var=var, rstd=rstd, d_mean=d_mu, d_rstd=d_rs, n_stat=n, y_mag=y_mag, y_n=1, y_cond=y_cond)
    if relu:
        near = pre.abs() <= NORM_TIE_C * U32 * y_mag + y_cond
        mask = (pre > 0).to(x.dtype)
        out.update(y=pre.clamp(min=0), near_zero=near)
    else:
        near = torch.zeros_like(pre, dtype=torch.bool)
        mask = torch.ones_like(pre)
        out.update(y=pre, near_zero=near)
    out["near_zero_share"] = float(near.double().mean()) if near.numel() else 0.0
    if dy is None:
        return out
    dyp = dy * mask
    g = w * dyp

    def bwd(m, s):
        xh = (x - m) * s
        return s * (g - g.mean(stat_dims, keepdim=True) - xh * (g * xh).mean(stat_dims, keepdim=True)), dyp * xh

    dx, t = bwd(mu, rstd)
    dx_cond, t_cond = sens(bwd)
    xh = (x - mu) * rstd
    ga = g.abs()
    dx_mag = rstd * (ga + ga.mean(stat_dims, keepdim=True) + xh.abs() * (ga * xh.abs()).mean(stat_dims, keepdim=True))
    dw_cond = t_cond.sum(par_dims, keepdim=True)
    db_cond = torch.zeros_like(dw_cond)
    if relu:
        nz = near.to(x.dtype)
        a1 = (nz * (w * dy).abs()).sum(stat_dims, keepdim=True) / n
        a2 = (nz * (w * dy * xh).abs()).sum(stat_dims, keepdim=True) / n
        dx_cond = dx_cond + rstd * (a1 + xh.abs() * a2)
        dw_cond = dw_cond + (nz * (dy * xh).abs()).sum(par_dims, keepdim=True)
        db_cond = db_cond + (nz * dy.abs()).sum(par_dims, keepdim=True)
    n_par = 1
    for d in par_dims:
        n_par *= x.shape[d]
    out.update(dx=dx, dx_mag=dx_mag, dx_n=n, dx_cond=dx_cond,
               dresidual=dyp, dresidual_mag=dyp.abs(), dresidual_n=1, dresidual_cond=torch.zeros_like(dyp),
               dweight=t.sum(par_dims, keepdim=True), dweight_mag=t.abs().sum(par_dims, keepdim=True), dweight_n=n_par,
               dweight_cond=dw_cond,
               dbias=dyp.sum(par_dims, keepdim=True), dbias_mag=dyp.abs().sum(par_dims, keepdim=True), dbias_n=n_par,
               dbias_cond=db_cond)
    return out


_NORM_OUTS = ("y", "dx", "dresidual", "dweight", "dbias")


def _norm_result(core, shape, par_shape, keep):
    """Reshape the core's outputs: y / dx / dresidual to `shape`, dweight / dbias to `par_shape`; `keep` names the outputs."""
    res = {"near_zero": core["near_zero"].reshape(shape), "near_zero_share": core["near_zero_share"]}
    for k in keep:
        if k not in core:
            continue
        shp = par_shape if k in ("dweight", "dbias") else shape
        for t in ("", "_mag", "_cond"):
            res[k + t] = core[k + t].reshape(shp)
        res[k + "_n"] = core[k + "_n"]
    return res


def batchnorm_fp64(x, residual, w, b, running_mean, running_var, momentum, eps, relu, dy):
    """relu?(BatchNorm(x) + residual?) in training mode over rows x [M, C], statistics per channel over the M rows, with its
    gradients for the upstream dy (or None: forward only) and the updated running statistics: running_mean' = (1 - momentum)
    running_mean + momentum mu, running_var' likewise with the unbiased var M / (M - 1).  Returns y, dx, dresidual (with a
    residual), dweight, dbias, running_mean, running_var, each with `_mag`, `_n`, `_cond`; near_zero [M, C] bool and
    near_zero_share (see the section comment)."""
    f64 = lambda t: None if t is None else t.detach().to(torch.float64)   # noqa: E731
    x64 = f64(x)
    m, c = x64.shape
    core = _norm_fp64(x64, (0,), (0,), f64(w).view(1, c), f64(b).view(1, c), f64(residual), eps, relu, f64(dy))
    res = _norm_result(core, (m, c), (c,), [k for k in _NORM_OUTS if k != "dresidual" or residual is not None])
    rm, rv = f64(running_mean).view(1, c), f64(running_var).view(1, c)
    unb = m / max(m - 1, 1)

    def running(mu, s):
        return (1 - momentum) * rm + momentum * mu, (1 - momentum) * rv + momentum * unb * (s ** -2 - eps)

    new_rm, new_rv = running(core["mean"], core["rstd"])
    zero = torch.zeros_like(core["mean"])
    _, j1 = torch.func.jvp(running, (core["mean"], core["rstd"]), (core["d_mean"], zero))
    _, j2 = torch.func.jvp(running, (core["mean"], core["rstd"]), (zero, core["d_rstd"]))
    mags = ((1 - momentum) * rm.abs() + momentum * core["mean"].abs(), (1 - momentum) * rv.abs() + momentum * unb * core["var"])
    for k, v, mag, a, bb in zip(("running_mean", "running_var"), (new_rm, new_rv), mags, j1, j2):
        res.update({k: v.view(c), k + "_mag": mag.view(c), k + "_n": 1, k + "_cond": (a.abs() + bb.abs()).view(c)})
    return res


def groupnorm_fp64(x, w, b, groups, eps, dy):
    """GroupNorm of a channels-last x [B, rows, C]: statistics per (sample, group) over rows x C / groups, affine per
    channel.  Returns y, dx, dweight, dbias with `_mag`, `_n`, `_cond` (dx_n = rows * C / groups, dweight_n = B * rows)."""
    x64 = x.detach().to(torch.float64)
    bsz, rows, c = x64.shape
    cpg = c // groups
    v = lambda t: t.detach().to(torch.float64).view(1, 1, groups, cpg)   # noqa: E731
    core = _norm_fp64(x64.view(bsz, rows, groups, cpg), (1, 3), (0, 1), v(w), v(b), None, eps, False,
                      None if dy is None else dy.detach().to(torch.float64).reshape(bsz, rows, groups, cpg))
    return _norm_result(core, (bsz, rows, c), (c,), ("y", "dx", "dweight", "dbias"))


def add_layernorm_fp64(x, residual, w, b, eps, dy):
    """LayerNorm(z) over the last axis of z = fp32(x + residual): the fp32 sum is the op's saved tensor and so part of its
    definition; it is formed in fp32 and everything after it in float64.  Returns y, dx, dresidual (with a residual: the same
    values as dx), dweight, dbias with `_mag`, `_n`, `_cond` (dx_n = C, dweight_n = rows), and z (float64)."""
    c = x.shape[-1]
    z = x.detach().float() if residual is None else x.detach().float() + residual.detach().float()
    z64 = z.to(torch.float64).reshape(-1, c)
    v = lambda t: t.detach().to(torch.float64).view(1, c)   # noqa: E731
    core = _norm_fp64(z64, (1,), (0,), v(w), v(b), None, eps, False,
                      None if dy is None else dy.detach().to(torch.float64).reshape(-1, c))
    res = _norm_result(core, tuple(x.shape), (c,), ("y", "dx", "dweight", "dbias"))
    res["z"] = z64.reshape(x.shape)
    if residual is not None and dy is not None:
        for t in ("", "_mag", "_cond", "_n"):
            res["dresidual" + t] = res["dx" + t]
    return res


# ---- attention: softmax(scale Q K^T, masked) V and its gradients (csrc/attention.hip) -----------------------------------------
# Written out from the definition: s = scale q k^T, a masked pair takes no part, lse = log sum_j exp(s_ij), p = exp(s - lse),
# out = p v; backward: dv = p^T dO, dP = dO v^T, D_i = sum_x dO_ix out_ix, dS = p (dP - D), dq = scale dS k, dk = scale dS^T q.
# A query with no allowed key has p = 0 throughout: out, dq and its share of dk and dv are exactly 0, lse = -inf.  Nothing of
# efg_amd and no torch softmax / logsumexp / autograd is used.
# `_mag` is the same sum over absolute values, `_n` the number of terms of the element's last sum (allowed keys of the query for
# out and dq, allowed queries of the key for dk and dv) and `_cond` an ABSOLUTE allowance for assert_elementwise's `geo64`.  A
# softmax is ill-conditioned in its logits: ANY fp32 evaluation from the fixed fp32 inputs rounds the logit, the row's
# log-sum-exp (or max and sum) and the exponential, and a change e of the exponent moves p by p e.  With u = 2^-24 and d the head
# width, independent roundings added in quadrature, the exponent of an allowed pair is uncertain by
#   delta_ij = u (sqrt(d) scale sqrt(sum_x q_ix^2 k_jx^2)    the d products of the dot product, each rounded once
#               + |s_ij|                                      the rounded factor scale (* log2 e) folded into one operand
#               + |lse_i|                                     the log-sum-exp stored (or the running max held) in fp32
#               + |s_ij - lse_i|                              the subtraction's result
#               + 2)                                          a 1-ulp exp (2^-23 relative) -- delta_ij = 0 for a masked pair
# The row's normaliser is the sum of the p_ij: a_i = sqrt(sum_j (p_ij delta_ij)^2) in relative terms.  So p_ij carries
# F_ij = p_ij (delta_ij + a_i), and out_cond = sqrt(F^2 v^2), dv_cond = sqrt(F^2^T dO^2), lse_cond = a_i + 2 u |lse_i| (the log
# and the stored value).  dS = p (dP - D) carries
#   E_ij = |dS_ij| (delta_ij + a_i)                                       the error of p_ij
#        + p_ij sqrt(sum_j' (dS_ij' delta_ij')^2)                         D_i = sum_j p_ij dP_ij moves with every p_ij' of the row
#        + p_ij (sqrt(d) u sqrt(sum_x dO_ix^2 v_jx^2) + Derr_i)           the d products of dP_ij; the rounded D_i
#        + 2 u |dS_ij|                                                    the subtraction and the product
# with Derr_i = sqrt(sum_x (|dO_ix| (out_cond + sqrt(n) u out_mag)_ix)^2) + sqrt(d) u sqrt(sum_x (dO_ix out_ix)^2): D_i is taken
# from the ROUNDED fp32 out and is a sum of d products.  dq_cond = scale sqrt(E^2 k^2), dk_cond = scale sqrt(E^2^T q^2).  `_cond`
# never sees a kernel's output.  Unlike the worst-case sums of the detection-loss and norm sections it is a QUADRATURE -- the size
# of one standard deviation when every rounding is as large as it can be -- so a test passes geo64 = c * cond: the bar is
# c (sqrt(n) 2^-24 |terms| + cond), one constant over both root-sum-square estimates (attention_fp64_cases.check_against).
def attention_fp64(q, k, v, grad_out, scale, mask=None):
    """Scaled-dot-product attention and its gradients in float64.  q, grad_out [B, H, Sq, D], k, v [B, H, Sk, D] (any strides),
    mask bool [Sq, Sk] (True = not attended) or None.  Returns a dict: out [B, H, Sq, D], lse [B, H, Sq], dq, dk, dv like q, k, v,
    each with `_mag`, `_n` and `_cond` (see the section comment); live [Sq] bool: queries with at least one allowed key."""
    q64, k64, v64, g64 = (t.detach().to(torch.float64) for t in (q, k, v, grad_out))
    dev = q64.device
    sq, sk, d = q64.shape[2], k64.shape[2], q64.shape[3]
    scale = float(scale)
    allowed = torch.ones(sq, sk, dtype=torch.bool, device=dev) if mask is None else ~mask.to(dev)
    al = allowed.to(torch.float64)
    live = allowed.any(1)
    lv = live.view(1, 1, sq, 1)
    kt, vt = k64.transpose(-1, -2), v64.transpose(-1, -2)
    s = scale * (q64 @ kt)                                                          # [B, H, Sq, Sk]
    s_m = s.masked_fill(~allowed, -math.inf)
    m0 = torch.where(lv, s_m.max(-1, keepdim=True).values, torch.zeros((), dtype=torch.float64, device=dev))
    e = torch.exp(s_m - m0)                                                         # a masked pair: exp(-inf) = 0
    l = e.sum(-1, keepdim=True)
    p = e / l.clamp_min(1e-300)                                                     # a dead row: 0 / tiny = 0
    lse0 = (m0 + torch.log(l.clamp_min(1e-300))) * lv                               # 0 in dead rows
    lse = torch.where(lv, lse0, torch.full((), -math.inf, dtype=torch.float64, device=dev)).squeeze(-1)
    out = p @ v64
    n_q = al.sum(1).view(1, 1, sq, 1)
    n_k = al.sum(0).view(1, 1, sk, 1)

    delta = U32 * (math.sqrt(d) * scale * torch.sqrt((q64 ** 2) @ (kt ** 2)) + s.abs() + lse0.abs() + (s - lse0).abs() + 2.0) * al
    a = torch.sqrt(((p * delta) ** 2).sum(-1, keepdim=True))
    f2 = (p * (delta + a)) ** 2
    out_mag = p @ v64.abs()
    out_cond = torch.sqrt(f2 @ v64 ** 2)
    dv = p.transpose(-1, -2) @ g64
    dv_mag = p.transpose(-1, -2) @ g64.abs()
    dv_cond = torch.sqrt(f2.transpose(-1, -2) @ g64 ** 2)
    lse_cond = (a + 2 * U32 * lse0.abs()).squeeze(-1)

    dp = g64 @ vt
    dd = (g64 * out).sum(-1, keepdim=True)
    ds = p * (dp - dd)
    d_err = torch.sqrt(((g64.abs() * (out_cond + torch.sqrt(n_q.clamp_min(1.0)) * U32 * out_mag)) ** 2).sum(-1, keepdim=True)) \
        + math.sqrt(d) * U32 * torch.sqrt(((g64 * out) ** 2).sum(-1, keepdim=True))
    err = ds.abs() * (delta + a) + p * torch.sqrt(((ds * delta) ** 2).sum(-1, keepdim=True)) \
        + p * (math.sqrt(d) * U32 * torch.sqrt((g64 ** 2) @ (vt ** 2)) + d_err) + 2 * U32 * ds.abs()
    e2 = err ** 2
    dq = scale * (ds @ k64)
    dq_mag = scale * (ds.abs() @ k64.abs())
    dq_cond = scale * torch.sqrt(e2 @ k64 ** 2)
    dk = scale * (ds.transpose(-1, -2) @ q64)
    dk_mag = scale * (ds.abs().transpose(-1, -2) @ q64.abs())
    dk_cond = scale * torch.sqrt(e2.transpose(-1, -2) @ q64 ** 2)
    return dict(out=out, out_mag=out_mag, out_n=n_q, out_cond=out_cond,
                lse=lse, lse_mag=torch.zeros_like(lse), lse_n=1, lse_cond=lse_cond,
                dq=dq, dq_mag=dq_mag, dq_n=n_q, dq_cond=dq_cond,
                dk=dk, dk_mag=dk_mag, dk_n=n_k, dk_cond=dk_cond,
                dv=dv, dv_mag=dv_mag, dv_n=n_k, dv_cond=dv_cond, live=live)
