"""Split-precision products of csrc/gemm_split_bf16.h through the C ABI, written once for the two arms.

`bind(prefix)` gives the five functions of one arm (`efg_gemm_bf16x3` or `efg_gemm_bf16x6`: six C symbols each, same
signatures); operators/gemm_bf16x3.py and operators/gemm_bf16x6.py are what the rest of the package imports.  The packed
layouts of the arms differ (2 or 3 pieces per element): a buffer packed by one is not an argument for the other."""
import torch

from .. import _lib


def bind(prefix):
    """(pack, pack_linear, pack_linear_both, gemm, wgrad) on the C symbols `prefix`_*."""

    # (the symbol names are put together here, once: the packers are launch-bound, 10 us a call, and a helper that built the
    # name and loaded the library handle per symbol cost them 0.6-0.9 us)
    pack_bytes_, pack_f32_, pack_linear_f32_, gemm_f32_, wgrad_bytes_, wgrad_f32_ = (
        prefix + s for s in ("_pack_bytes", "_pack_f32", "_pack_linear_f32", "_f32", "_wgrad_workspace_bytes", "_wgrad_f32"))

    def pack(w, k, n, stride_k, stride_n):
        """Split B(kk, nn) = w.flatten()[kk * stride_k + nn * stride_n] into the MFMA lane order (device buffer)."""
        lib = _lib.lib()
        out = torch.empty(getattr(lib, pack_bytes_)(k, n), dtype=torch.uint8, device=w.device)
        _lib.check(getattr(lib, pack_f32_)(_lib.ptr(w), stride_k, stride_n, k, n, _lib.ptr(out), _lib.stream()))
        return out

    def pack_linear(weight, transposed):
        """weight [out, in] of an nn.Linear.  transposed=False: B = W^T [in, out] (y = x W^T); True: B = W [out, in]
        (dx = dy W)."""
        w = weight.contiguous()
        o, i = w.shape
        return pack(w, i, o, 1, i) if not transposed else pack(w, o, i, i, 1)

    def pack_linear_both(weight):
        """(B = W^T for y = x W^T, B = W for dx = dy W) of an nn.Linear weight [out, in], one launch."""
        w = weight.contiguous()
        o, i = w.shape
        lib = _lib.lib()
        fwd = torch.empty(getattr(lib, pack_bytes_)(i, o), dtype=torch.uint8, device=w.device)
        dgr = torch.empty(getattr(lib, pack_bytes_)(o, i), dtype=torch.uint8, device=w.device)
        _lib.check(getattr(lib, pack_linear_f32_)(_lib.ptr(w), o, i, _lib.ptr(fwd), _lib.ptr(dgr), _lib.stream()))
        return fwd, dgr

    def gemm(a, packed, n, bias=None, relu=False):
        """a [m, k] fp32 (rows contiguous) x packed B [k, n] -> [m, n] fp32."""
        assert a.dim() == 2 and a.dtype == torch.float32 and a.stride(1) == 1
        m, k = a.shape
        c = torch.empty((m, n), dtype=torch.float32, device=a.device)
        _lib.check(getattr(_lib.lib(), gemm_f32_)(a.data_ptr(), m, k, a.stride(0), _lib.ptr(packed), n,
                                                  _lib.ptr(bias) if bias is not None else None, 1 if relu else 0,
                                                  _lib.ptr(c), n, _lib.stream()))
        return c

    def wgrad(g, x):
        """g [m, n] (grad_output), x [m, k] (input), fp32 rows contiguous -> g^T x [n, k] (an nn.Linear's weight gradient)."""
        assert g.dim() == 2 and x.dim() == 2 and g.shape[0] == x.shape[0] and g.stride(1) == 1 and x.stride(1) == 1
        m, n = g.shape
        k = x.shape[1]
        lib = _lib.lib()
        out = torch.empty((n, k), dtype=torch.float32, device=g.device)
        ws_bytes = getattr(lib, wgrad_bytes_)(m, n, k)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=g.device)
        _lib.check(getattr(lib, wgrad_f32_)(g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0), m, n, k, _lib.ptr(out),
                                            _lib.ptr(ws), ws_bytes, _lib.stream()))
        return out

    return pack, pack_linear, pack_linear_both, gemm, wgrad
