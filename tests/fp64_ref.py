"""Plain float64 references for the sparse convolution and the fused box attention, and an element-wise error bar.

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


def sample_fp64(value, shapes, starts, loc, attn, grad_out=None, geo_ulps=GEO_ULPS):
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
    the number of (point, corner) entries summed into each grad_value row."""
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
        for cx, cy, wgt, dwx, dwy in _corners(px, py):
            inside = ((cx >= 0) & (cx < wl) & (cy >= 0) & (cy < hl)).to(torch.float64)
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
