"""Thin torch-tensor wrappers over the C-ABI (device pointers + sizes + current HIP stream).

torch is used for device memory and streams only; every arithmetic op on the path is a HIP kernel from
libullava_hip.so.  Activations are 16-bit (bf16 or fp16: every kernel exists in both builds, picked by the dtype of the op's first
operand; the other operands must match), row-major, last dim contiguous.
"""
import functools
import weakref
from typing import NamedTuple, Optional


import torch

from . import _lib

BF16 = torch.bfloat16
F16 = torch.float16
F32 = torch.float32
# entry-point suffix by element type: the two 16-bit builds of every dtype-dependent kernel, and the fp32 build of the inference path
# (csrc/f32.hip: `--dtype fp32`, plain kernels on the exact fp32 matrix instruction -- a correctness path, no fused / tiled fast paths)
_SFX = {BF16: "bf16", F16: "f16", F32: "f32"}
_D = _lib.DEFINES                                           # every flag / code / limit below is the header's #define ULL_* of that name
DT_CODE = {torch.float32: _D["ULL_DT_F32"], BF16: _D["ULL_DT_BF16"], F16: _D["ULL_DT_F16"]}      # the dtype-coded entry points
EPI_BIAS, EPI_QGELU, EPI_GELU, EPI_RELU, EPI_RESID, EPI_SWIGLU, EPI_F32 = (
    _D["ULL_EPI_" + n] for n in ("BIAS", "ACT_QUICK_GELU", "ACT_GELU", "ACT_RELU", "RESID", "SWIGLU", "OUT_F32"))
EPI_BIAS_ROUNDED = _D["ULL_EPI_BIAS_ROUNDED"]
ACTS = {None: 0, "quick_gelu": EPI_QGELU, "gelu": EPI_GELU, "relu": EPI_RELU}


_ZEROS = {}


def _zeros(device):
    z = _ZEROS.get(device)
    if z is None:
        z = _ZEROS[device] = torch.zeros(256, device=device, dtype=BF16)
    return z


def vt_unpermute_index(pitch: int) -> torch.Tensor:
    """index so that vt[..., idx] is in natural key order (inverse of the 32-key block permutation of transpose_v)."""
    key = torch.arange(pitch)
    w = key % 32
    a, g, r = w // 16, (w % 16) // 4, w % 4
    return (key // 32) * 32 + 8 * g + 4 * a + r


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _copy_sfx(dtype, D: int):
    """(entry suffix, row width in that entry's elements) of a PURE data-movement kernel: fp32 rows go through the 16-bit kernel as rows of
    twice as many 16-bit elements (the same bytes; csrc/f32.hip has no copy kernels of its own)."""
    if dtype == F32:
        if D % 4:
            raise RuntimeError("u-llava_amd: fp32 rows must be a multiple of 4 elements wide")
        return "bf16", 2 * D
    return _SFX[dtype], D


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, name: str, dtype=None):
    """dtype None: any 16-bit element type with a kernel build (bf16 / fp16); otherwise exactly `dtype` (the op's other operands
    must match its first one -- there are no mixed-dtype kernels)."""
    if not t.is_cuda:
        raise RuntimeError(f"u-llava_amd: `{name}` must live on the GPU (no CPU path exists)")
    if dtype is None:
        if t.dtype not in _SFX:
            raise RuntimeError(f"u-llava_amd: `{name}` must be torch.bfloat16, torch.float16 or torch.float32, got {t.dtype}")
    elif t.dtype != dtype:
        raise RuntimeError(f"u-llava_amd: `{name}` must be {dtype}, got {t.dtype}")
    if t.dim() and t.stride(-1) != 1:
        raise RuntimeError(f"u-llava_amd: `{name}` must be contiguous in its last dim")


def _rows(t: torch.Tensor):
    """View [*, D] as rows with one row stride; returns (rows, ld)."""
    if t.dim() == 1:
        return 1, t.shape[0]
    if t.dim() == 2:
        return t.shape[0], t.stride(0)
    if t.is_contiguous():
        return t.numel() // t.shape[-1], t.shape[-1]
    # a [..., :D] view of a wider buffer (a [B, S, D] slice of packed rows): the leading dims still fold onto ONE row stride
    if t.stride(-1) != 1 or any(t.stride(i) != t.shape[i + 1] * t.stride(i + 1) for i in range(t.dim() - 2)):
        raise RuntimeError("u-llava_amd: >2-D operands must be contiguous, or rows of one common pitch")
    return t.numel() // t.shape[-1], t.stride(-2)


EPI_W_TILED = _D["ULL_EPI_W_TILED"]
_TILED = {}          # data_ptr of a row-major weight -> (weakref to it, its tile-major copy, the weight's ._version the copy was made from)


def tile_major(w: torch.Tensor) -> torch.Tensor:
    """[N, K] (K % 64 == 0) -> [ceil(N/256), K/64, 256, 64] contiguous: the ULL_EPI_W_TILED layout of ull_gemm_bf16."""
    N, K = w.shape
    Np = (N + 255) // 256 * 256
    if Np != N:
        w = torch.cat([w, w.new_zeros(Np - N, K)])
    return w.view(Np // 256, 256, K // 64, 64).permute(0, 2, 1, 3).contiguous()


def register_tiled(w: torch.Tensor) -> None:
    """Keep a tile-major copy of a weight for the prefill-shape GEMM (the row-major original still feeds the decode GEMV)."""
    if w.dim() == 2 and w.shape[1] % 64 == 0 and w.shape[0] >= 512 and w.shape[1] >= 128 and w.is_contiguous() and w.dtype != F32:
        ptr = w.data_ptr()
        _TILED[ptr] = [weakref.ref(w, lambda _r, _p=ptr: _TILED.pop(_p, None) if (_TILED.get(_p) or (None,))[0] is _r else None),
                       tile_major(w.detach()), w._version]    # the copy is dropped when the weight tensor dies


def _tiled_of(w: torch.Tensor):
    """The tile-major copy of `w`, or None.  The copy describes the weight AS IT WAS when the copy was made: an in-place update since
    (an optimizer step's `p.copy_`, `load_state_dict`, `merge_lora`) bumps `w._version`, and the copy is then re-made from the live
    values before it is handed out -- a training run must never multiply by step-0 weights."""
    e = _TILED.get(w.data_ptr())
    if e is None:
        return None
    if e[0]() is not w:
        _TILED.pop(w.data_ptr(), None)       # the address was recycled by another tensor
        return None
    if e[2] != w._version:
        # a NEW tensor, not copy_: a copy first made under torch.inference_mode() (the reference wraps generate / evaluate in it,
        # inference_ullava_core.py:72, models/ullava.py:349) is an inference tensor and may not be updated in place outside that mode
        # ... in place where that is allowed (a training run re-tiles every weight after every optimizer step: no allocator churn)
        N, K = w.shape
        if not e[1].is_inference() and not torch.is_inference_mode_enabled() and N % 256 == 0 and tuple(e[1].shape) == (N // 256, K // 64, 256, 64):
            with torch.no_grad():
                e[1].copy_(w.detach().view(N // 256, 256, K // 64, 64).permute(0, 2, 1, 3))
        else:
            e[1] = tile_major(w.detach())
        e[2] = w._version
    return e[1]


def unregister_tiled(w: torch.Tensor) -> None:
    """Drop the tile-major copy of `w` now (a weight whose storage is being released while the tensor object lives on)."""
    e = _TILED.get(w.data_ptr())
    if e is not None and e[0]() is w:
        del _TILED[w.data_ptr()]


# ---- FP8 (e4m3) weight-only storage (UllavaCoreForCausalLM.quantize_weights) ----------------------------------------------------------
class Fp8Weight:
    """A Linear weight [N, K] as e4m3fn codes (uint8 [N, K]) plus one fp32 power-of-two scale per row: dequant = float(code) * scale, exactly
    a bf16 value.  `linear` / `linear_qkv_rope` / `linear_qkv_rope_append` take it in place of a bf16 weight and compute exactly what they
    compute on the dequantized bf16 weight (the fp8 forms of the GEMV / skinny kernels at decode shapes; dequantize + the bf16 GEMM at
    prefill shapes).  Immutable once built.

    What the Linear dispatch needs of a quantized weight, here and on Mxfp4Weight: `fmt_name`, `wf` (its ULL_WF_* code), `route_pitch` (the row
    pitch `_linear_route` sees), `c_args()` (the weight arguments of a *_wq_bf16 entry / the fields of an ull_linear) and `dequantize_into`."""
    __slots__ = ("codes", "scales", "_kpad")
    fmt_name, wf = "fp8", _lib.WF_FP8

    def __init__(self, codes: torch.Tensor, scales: torch.Tensor):
        if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.stride(1) != 1 or scales.dtype != F32 or scales.shape != (codes.shape[0],):
            raise RuntimeError("u-llava_amd.Fp8Weight: codes uint8 [N, K] (rows contiguous), scales fp32 [N]")
        self.codes, self.scales = codes, scales
        self._kpad = None                    # a8_codes(): the aligned, zero-padded copy (tiny test models and views only; real weights never need it)

    @property
    def shape(self):
        return self.codes.shape

    @property
    def device(self):
        return self.codes.device

    def nbytes(self) -> int:
        return self.codes.numel() + 4 * self.scales.numel()

    @property
    def route_pitch(self) -> int:
        return self.codes.stride(0)          # code bytes = elements

    def a8_codes(self) -> torch.Tensor:
        """The codes as the 16-byte loads of the W8A8 kernels can take them: `codes` itself when K is a whole number of 128-code K-tiles and
        the rows are 16-byte aligned, else a contiguous copy zero-padded to K % 128 == 0, made once and kept."""
        c = self.codes
        if c.size(1) % A8W8_BK or c.stride(0) % 16 or c.data_ptr() % 16:
            if self._kpad is None:
                self._kpad = torch.nn.functional.pad(c, (0, -c.size(1) % A8W8_BK)).contiguous()
            c = self._kpad
        return c

    def c_args(self):
        """(wfmt, Q, ldq, scales, lds): lds is unused."""
        return self.wf, self.codes.data_ptr(), self.codes.stride(0), self.scales.data_ptr(), 0

    def dequantize_into(self, out: torch.Tensor, tiled: bool) -> None:
        N, K = self.shape
        _lib.call("ull_dequantize_rows_fp8_bf16", _p(self.codes), self.codes.stride(0), _p(self.scales), N, K, _p(out), int(tiled), _stream())


def quantize_fp8(w: torch.Tensor) -> Fp8Weight:
    """Per-row e4m3 quantization of a bf16 weight [N, K] on the GPU (ull_quantize_rows_fp8_bf16): the row's scale is 2^s with s the smallest
    integer such that amax|w| * 2^-s <= 448 (0 for an all-zero row); codes = e4m3fn(w * 2^-s), round to nearest even -- bit-identical to
    torch's CPU cast `(w.float() * 2**-s).to(torch.float8_e4m3fn)`."""
    _chk(w, "w", BF16)
    if w.dim() != 2:
        raise RuntimeError("u-llava_amd.quantize_fp8: w must be 2-D")
    N, K = w.shape
    codes = torch.empty(N, K, device=w.device, dtype=torch.uint8)
    scales = torch.empty(N, device=w.device, dtype=F32)
    _lib.call("ull_quantize_rows_fp8_bf16", _p(w), w.stride(0), N, K, _p(codes), _p(scales), _stream())
    return Fp8Weight(codes, scales)


def dequantize(q, tiled: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dequant(q) of an Fp8Weight / Mxfp4Weight as bf16: [N, K] row-major, or (tiled) the ULL_EPI_W_TILED layout `tile_major` produces."""
    N, K = q.shape
    rows = -(-N // 256) * 256 if tiled else N
    if out is None:
        out = torch.empty(rows * K, device=q.device, dtype=BF16)
    elif out.dtype != BF16 or out.numel() < rows * K or not out.is_contiguous():
        raise RuntimeError(f"u-llava_amd.dequantize_{q.fmt_name}: `out` must be a contiguous bf16 buffer of at least the result's size")
    q.dequantize_into(out, tiled)
    return out[:rows * K].view(rows // 256, K // 64, 256, 64) if tiled else out[:N * K].view(N, K)


dequantize_fp8 = dequantize_mxfp4 = dequantize


# ---- MXFP4 weight-only storage (UllavaCoreForCausalLM.quantize_weights("mxfp4")) -------------------------------------------------------
_MX_PERM = {}        # (K, device) -> (code byte index, scale byte index): resident position of every standard-layout byte of a row


def _mx_perm(K: int, device):
    """Index tensors of the resident layout (include/ullava_hip.h): resident[:, idx] = standard.  A chunk is 8 elements (4 code bytes), a
    superblock 256 chunks; inside whole superblock b chunk b * 256 + g * 64 + l sits at byte b * 1024 + l * 16 + g * 4, and the scale of block
    b * 64 + g * 16 + j at byte b * 64 + j * 4 + g; the rest of the row keeps the standard order."""
    key = (K, str(device))
    e = _MX_PERM.get(key)
    if e is None:
        nsb = K // 2048
        c = torch.arange(K // 8, device=device)
        cpos = torch.where(c < nsb * 256, (c >> 8) * 1024 + (c & 63) * 16 + ((c >> 6) & 3) * 4, c * 4)
        cidx = (cpos[:, None] + torch.arange(4, device=device)).reshape(-1)
        b = torch.arange(K // 32, device=device)
        sidx = torch.where(b < nsb * 64, (b >> 6) * 64 + (b & 15) * 4 + ((b >> 4) & 3), b)
        e = _MX_PERM[key] = (cidx, sidx)
    return e


class Mxfp4Weight:
    """A Linear weight [N, K] (K % 32 == 0) in the OCP microscaling format MXFP4: e2m1 codes, two per byte, plus one E8M0 scale byte per row
    and block of 32 consecutive K elements; dequant = e2m1 * 2^(scale - 127), exactly a bf16 value.  The object holds the RESIDENT layout
    the decode kernels read (codes uint8 [N, K / 2], scales uint8 [N, K / 32 rounded up to a multiple of 4]): the standard layout
    (`to_standard()`: codes [N, K / 2] with element 2i in the low nibble -- torch.float4_e2m1fn_x2 -- and scales [N, K / 32]) with the bytes
    of each row permuted, see include/ullava_hip.h.  `linear` / `linear_qkv_rope` / `linear_qkv_rope_append` take it in place of a bf16
    weight and compute exactly what they compute on the dequantized bf16 weight.  Immutable once built."""
    __slots__ = ("codes", "scales", "K", "_kpad")
    fmt_name, wf = "mxfp4", _lib.WF_MXFP4

    def __init__(self, codes: torch.Tensor, scales: torch.Tensor, K: int):
        if (codes.dtype != torch.uint8 or codes.dim() != 2 or K % 32 or codes.shape[1] != K // 2 or not codes.is_contiguous() or
                scales.dtype != torch.uint8 or scales.shape != (codes.shape[0], self.scale_pitch(K)) or not scales.is_contiguous()):
            raise RuntimeError("u-llava_amd.Mxfp4Weight: codes uint8 [N, K / 2], scales uint8 [N, K / 32 rounded up to 4], contiguous, K % 32 == 0")
        self.codes, self.scales, self.K = codes, scales, K
        self._kpad = None                    # linear_w4a8: (codes, scales) padded to K % 128 == 0 (tiny test models only; real K never needs it)

    @staticmethod
    def scale_pitch(K: int) -> int:
        return -(-(K // 32) // 4) * 4

    @property
    def shape(self):
        return torch.Size((self.codes.shape[0], self.K))

    @property
    def device(self):
        return self.codes.device

    def nbytes(self) -> int:
        return self.codes.numel() + self.scales.numel()

    @property
    def route_pitch(self) -> int:
        return self.K                        # its rows are always whole

    def c_args(self):
        """(wfmt, Q, ldq, scales, lds)."""
        return self.wf, self.codes.data_ptr(), self.codes.stride(0), self.scales.data_ptr(), self.scales.stride(0)

    def dequantize_into(self, out: torch.Tensor, tiled: bool) -> None:
        N, K = self.shape
        _lib.call("ull_dequantize_rows_mxfp4_bf16", _p(self.codes), self.codes.stride(0), _p(self.scales), self.scales.stride(0), N, K, _p(out),
                  int(tiled), 1, _stream())

    def to_standard(self):
        """(codes uint8 [N, K / 2], scales uint8 [N, K / 32]) in the standard layout."""
        cidx, sidx = _mx_perm(self.K, self.device)
        return self.codes[:, cidx], self.scales[:, sidx]

    @classmethod
    def from_standard(cls, codes: torch.Tensor, scales: torch.Tensor) -> "Mxfp4Weight":
        if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() != 2 or scales.dim() != 2:
            raise RuntimeError("u-llava_amd.Mxfp4Weight.from_standard: codes uint8 [N, K / 2], scales uint8 [N, K / 32]")
        N, K = codes.shape[0], codes.shape[1] * 2
        if K % 32 or scales.shape != (N, K // 32):
            raise RuntimeError("u-llava_amd.Mxfp4Weight.from_standard: codes uint8 [N, K / 2], scales uint8 [N, K / 32], K % 32 == 0")
        cidx, sidx = _mx_perm(K, codes.device)
        rc = torch.empty_like(codes, memory_format=torch.contiguous_format)
        rc[:, cidx] = codes
        rs = torch.zeros(N, cls.scale_pitch(K), device=scales.device, dtype=torch.uint8)
        rs[:, sidx] = scales
        return cls(rc, rs, K)


def quantize_mxfp4(w: torch.Tensor) -> Mxfp4Weight:
    """MXFP4 quantization of a bf16 weight [N, K], K % 32 == 0, on the GPU (ull_quantize_rows_mxfp4_bf16): per row and block of 32 K elements
    the scale is 2^s with s the smallest integer such that amax * 2^-s <= 6 (0 for an all-zero block), clamped to [-125, 126]; an element is
    e2m1(w * 2^-s) rounded to nearest, ties to the even code (at s = 126 saturating at the code of 3: 4 * 2^126 is no float).  Weight-only round-to-nearest, no calibration."""
    if w.dim() != 2:
        raise RuntimeError("u-llava_amd.quantize_mxfp4: w must be 2-D")
    N, K = w.shape
    if K % 32:
        raise NotImplementedError(f"u-llava_amd.quantize_mxfp4: K must be a multiple of 32 (one scale per 32 elements), got {K}")
    _chk(w, "w", BF16)
    codes = torch.empty(N, K // 2, device=w.device, dtype=torch.uint8)
    lds = Mxfp4Weight.scale_pitch(K)
    scales = (torch.empty if lds == K // 32 else torch.zeros)(N, lds, device=w.device, dtype=torch.uint8)
    _lib.call("ull_quantize_rows_mxfp4_bf16", _p(w), w.stride(0), N, K, _p(codes), K // 2, _p(scales), lds, 1, _stream())
    return Mxfp4Weight(codes, scales, K)


QuantWeight = (Fp8Weight, Mxfp4Weight)      # the quantized weight types the Linear dispatch rule takes beside a 16-bit tensor

_WQ_SCRATCH = {}     # (device, stream) -> the bf16 buffer prefill-shape fp8 / mxfp4 Linears dequantize into (reused in stream order)


def _wq_scratch(device: torch.device, stream_id: int, numel: int) -> torch.Tensor:
    key = (device.index, stream_id)
    buf = _WQ_SCRATCH.get(key)
    if buf is None or buf.numel() < numel:
        with torch.cuda.device(device):
            buf = _WQ_SCRATCH[key] = torch.empty(numel, device=device, dtype=BF16)
    return buf


def _wq_dequant_for_gemm(q, M: int):
    """(row-major view, tile-major view or None) of dequant(q) in the stream's scratch, laid out as the bf16 GEMM would read the
    weight at this M: tile-major where a bf16 weight has its tile-major copy (register_tiled: K % 64 == 0) and the 256 x 256 path takes it."""
    N, K = q.shape
    tiled = _big(M, N, K) and K % 64 == 0
    buf = _wq_scratch(q.device, _stream(), (-(-N // 256) * 256 if tiled else N) * K)
    wd = dequantize(q, tiled=tiled, out=buf)
    if tiled:
        return buf[:N * K].view(N, K), wd          # (the row-major view only carries the shape: the GEMM reads the tile-major copy)
    return wd, None


def _weight_args(w):
    """(entry suffix, weight arguments) of a decode-shape entry (skinny GEMM, GEMV, GEMV + RMSNorm, q|k|v + RoPE + cache append): a 16-bit
    weight passes (pointer, row pitch), a quantized one (format, codes, row pitch, scales, row pitch) to the *_wq_bf16 form."""
    if isinstance(w, QuantWeight):
        return "wq_bf16", w.c_args()
    return _SFX[w.dtype], (w.data_ptr(), w.stride(0))


# ---- stream-K workspace: one fp32 scratch buffer per (device, stream) ---------------------------------------------------
# ull_gemm_bf16 splits a partial last round of 256x256 tiles along K into fp32 slabs in a CALLER-owned workspace.  Each HIP
# stream gets its own buffer here, so GEMMs running concurrently on two streams (RES forward / evaluate: SAM encoder beside
# CLIP + LLaMA) never share scratch.  Whether to split at all is host policy: K >= streamk_min_k (default 2048: below that the
# slab round trip costs more than the partial round it replaces); `streamk_policy(None)` turns the split off, which the model
# does while a second stream is filling the idle CUs of a partial round anyway.
_SK_WS = {}
_SK_MIN_K = [2048]


def _streamk_ws(device: torch.device, stream_id: int):
    key = (device.index, stream_id)
    ws = _SK_WS.get(key)
    if ws is None:
        with torch.cuda.device(device):
            ws = _SK_WS[key] = torch.empty(_lib.query("ull_gemm_streamk_ws_bytes"), device=device, dtype=torch.uint8)
    return ws


# Latency mode for single-image prefills (M < 1024): split-K in the 128x128 kernel.  OFF by default: it makes a sample's result depend on
# the batch it is computed in (the fp32 summation order of K changes with the split), and the path's invariant -- sample b of a batch of
# 32 equals the single-sample run bit for bit through every layer (tests/test_full_depth_gpu.py) -- is worth more than 5 ms of prefill.
# `with ops.small_m_split_k(True):` turns it on (C2 shape at batch 1: 16.9 -> 11.9 ms, 59 -> 84 images/s).  (Round 6: no environment variable
# reads this any more -- the product has no environment switches.)
_SMALL_M_SPLIT_K = [False]


class small_m_split_k:
    def __init__(self, on: bool):
        self.on = bool(on)

    def __enter__(self):
        self.prev = _SMALL_M_SPLIT_K[0]
        _SMALL_M_SPLIT_K[0] = self.on
        return self

    def __exit__(self, *exc):
        _SMALL_M_SPLIT_K[0] = self.prev
        return False


class streamk_policy:
    """with streamk_policy(min_k): ... -- K threshold of the stream-K tail inside the block (None = never split)."""

    def __init__(self, min_k: Optional[int]):
        self.min_k = min_k

    def __enter__(self):
        self.prev = _SK_MIN_K[0]
        _SK_MIN_K[0] = self.min_k
        return self

    def __exit__(self, *exc):
        _SK_MIN_K[0] = self.prev
        return False


# ---- the Linear dispatch rule: every route of `linear` / `linear_qkv_rope` is decided here ------------------------------------------------
class ActQuant(NamedTuple):
    """quantize_weights(activations=fmt, activation_scope=): "fp8_e4m3" (one scale per token, on an Fp8Weight) or "mxfp8_e4m3" / "mxfp4_e2m1" (one
    per block of 32, on an Mxfp4Weight); decode: also at the batched decode shapes ("prefill+decode", fp8 only).  decode_fmt:
    quantize_weights(decode_activations=): the format of the activations at the batched decode shapes, chosen on its own ("mxfp8_e4m3" on an
    Mxfp4Weight; fmt may then be None: a weight-only prefill with W4A8 decode steps).  None in its place means weight-only."""
    fmt: Optional[str]
    decode: bool = False
    decode_fmt: Optional[str] = None


A8W8_BK, A8W8_SKINNY_MAX_M, W4A8_SKINNY_MAX_M = _D["ULL_A8W8_BK"], _D["ULL_A8W8_SKINNY_MAX_M"], _D["ULL_W4A8_SKINNY_MAX_M"]
_ROUTES = {_D["ULL_ROUTE_" + r.upper()]: r for r in ("gemm", "gemv", "skinny", "a8w8", "w4a8", "a8w8_skinny", "w4a4", "w4a8_skinny")}
_WF = {None: _lib.WF_ELEM, "fp8": _lib.WF_FP8, "mxfp4": _lib.WF_MXFP4}
_AF = {"fp8_e4m3": _D["ULL_AF_FP8"], "mxfp8_e4m3": _D["ULL_AF_MXFP8"], "mxfp4_e2m1": _D["ULL_AF_MXFP4"]}


# The rule itself is csrc/linear_route.h, which the library's own callers (the coarse entries among them) apply; the three functions below ask
# the library once per distinct shape and keep the answer, so a warm path pays a dictionary hit, not a C call.
@functools.lru_cache(maxsize=None)
def _linear_route(M: int, N: int, K: int, ldw: int, tune: int, wfmt: Optional[str] = None, aq: Optional[ActQuant] = None):
    """(route, rms_first) of a Linear x [M, K] @ w.T, w [N, K] with row pitch ldw; wfmt: None for a 16-bit weight, else its `fmt_name`.
    route "gemm": the tiled GEMM; "gemv": the weight-streaming GEMV at decode shapes; "skinny": batched decode steps against LLaMA-sized
    weights on the matrix cores; "a8w8" (linear_a8w8) / "w4a8" (linear_w4a8) / "w4a4" (linear_w4a4): quantized activations where aq pairs with the weight format and
    the weight-only rule says "gemm"; "a8w8_skinny" (linear_a8w8_skinny): aq.decode on fp8 weights; "w4a8_skinny" (linear_w4a8_skinny):
    aq.decode_fmt "mxfp8_e4m3" on mxfp4 weights.
    rms_first: a requested RMSNorm is a launch of its own ahead of the Linear (False: the route's kernel fuses it)."""
    af = _D["ULL_AF_NONE"] if aq is None else _AF.get(aq.fmt, _D["ULL_AF_NONE"])
    a_decode = 0 if aq is None else _AF[aq.decode_fmt] if aq.decode_fmt is not None else int(aq.decode)
    r = _lib.query("ull_linear_route", M, N, K, ldw, _WF[wfmt], af, a_decode, tune)
    return _ROUTES[r & 255], bool(r >> 8)


def linear_route(M: int, w, act_quant: Optional[ActQuant] = None) -> str:
    """The route `linear` takes for M rows against the weight w (16-bit tensor / Fp8Weight / Mxfp4Weight) under act_quant."""
    wq = isinstance(w, QuantWeight)
    return _linear_route(M, w.shape[0], w.shape[1], w.route_pitch if wq else w.stride(0), 0, w.fmt_name if wq else None, act_quant)[0]


# the rule read as a boolean, for callers that ask about one A8 route (N and K are w's own)
a8w8_takes = lambda M, N, K, w: linear_route(M, w, ActQuant("fp8_e4m3")) == "a8w8"                          # noqa: E731
w4a8_takes = lambda M, N, K, w: linear_route(M, w, ActQuant("mxfp8_e4m3")) == "w4a8"                        # noqa: E731
w4a4_takes = lambda M, N, K, w: linear_route(M, w, ActQuant("mxfp4_e2m1")) == "w4a4"                        # noqa: E731
a8w8_decode_takes = lambda M, N, K, w: linear_route(M, w, ActQuant("fp8_e4m3", True)) == "a8w8_skinny"      # noqa: E731
w4a8_decode_takes = lambda M, N, K, w: linear_route(M, w, ActQuant(None, False, "mxfp8_e4m3")) == "w4a8_skinny"    # noqa: E731


@functools.lru_cache(maxsize=None)
def _gemm_plan(M: int, N: int, K: int, min_k: Optional[int], small_m: bool, small_m_split_k: bool):
    """(big, split) of a tiled GEMM (ull_gemm_plan).  big: it takes its 256 x 256 kernel and the weight's tile-major copy; split: it gets the
    workspace -- the stream-K tail of a big GEMM from K >= min_k on (None: never), or -- small_m: the kernel has the split, and
    small_m_split_k is on -- the split-K of a small-M one."""
    r = _lib.query("ull_gemm_plan", M, N, K, -1 if min_k is None else max(int(min_k), 0), small_m, small_m_split_k)
    return bool(r & 1), bool(r & 2)


def _big(M: int, N: int, K: int) -> bool:
    """`_gemm_plan`'s big, which depends on the shape alone."""
    return _gemm_plan(M, N, K, None, False, False)[0]


@functools.lru_cache(maxsize=None)
def decode_step_fused(T: int, D: int, hd: int) -> bool:
    """A generation step of T = B * S tokens at width D = H * hd runs RoPE and the cache append in the q|k|v GEMV's epilogue
    (linear_qkv_rope_append; the shape check of the coarse decode entry)."""
    return bool(_lib.query("ull_decode_step_fused", T, D, hd))


def _gemm_ws(device: torch.device, stream_id: int, big: bool, M: int, N: int, K: int, small_m: bool):
    """(pointer, bytes) of the fp32 workspace the tiled GEMM of `_gemm_plan` splits K into, or (None, 0).  big: `_big(M, N, K)`."""
    if not _gemm_plan(M, N, K, _SK_MIN_K[0], small_m, _SMALL_M_SPLIT_K[0])[1]:
        return None, 0
    ws = _streamk_ws(device, stream_id)
    return ws.data_ptr(), ws.numel()


def _epilogue(x: torch.Tensor, N: int, swiglu: bool, out_f32: bool, residual: Optional[torch.Tensor], out: Optional[torch.Tensor], dtype=None):
    """(out, flags, ldr) of a Linear on the rows x [..., K] (or their codes) with 16-bit type `dtype` (default: x's): `out`, allocated on x's
    leading dims unless given, the swiglu / out_f32 / residual flag bits, and the checked residual's row pitch (0 without one)."""
    if out is None:
        out = torch.empty(*x.shape[:-1], N // 2 if swiglu else N, device=x.device, dtype=F32 if out_f32 else dtype or x.dtype)
    flags = (EPI_SWIGLU if swiglu else 0) | (EPI_F32 if out_f32 else 0)
    ldr = 0
    if residual is not None:
        _chk(residual, "residual", dtype or x.dtype)
        flags |= EPI_RESID
        ldr = _rows(residual)[1]
    return out, flags, ldr


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
           residual: Optional[torch.Tensor] = None, swiglu: bool = False, out: Optional[torch.Tensor] = None,
           out_f32: bool = False, rms_w: Optional[torch.Tensor] = None, rms_eps: float = 0.0, tune: int = 0,
           bias_after_rounding: bool = False, act_quant: Optional[ActQuant] = None) -> torch.Tensor:
    """y = epilogue(x @ w.T).  x [..., K]; w [N, K] (nn.Linear layout).  swiglu: w is the 16-row interleaved gate/up pack.
    rms_w/rms_eps: apply LlamaRMSNorm to x first (fused into the GEMV prologue at decode shapes, a separate kernel otherwise).
    tune: ULL_GEMM_TUNE_* bits (tools/ only).  bias_after_rounding: y = round(round(x @ w.T) + bias) -- what at::linear computes
    for a NON-contiguous 3-D input (matmul + add_ instead of the fused addmm).
    w may be an `Fp8Weight` or an `Mxfp4Weight` (bf16 x only): the same result as on its dequantized bf16 weight, bit for bit.
    act_quant: quantize the activations too wherever `_linear_route` gives an A8 route (residual / swiglu / out / out_f32 / rms_w only)."""
    wq = isinstance(w, QuantWeight)
    if wq and x.dtype != BF16:
        raise RuntimeError(f"u-llava_amd.linear: {w.fmt_name} weights need bf16 activations, got {x.dtype}")
    _chk(x, "x")
    if not wq:
        _chk(w, "w", x.dtype)
    M, ldx = _rows(x)
    N, K = w.shape
    if x.shape[-1] != K:
        raise RuntimeError(f"u-llava_amd.linear: K mismatch {x.shape[-1]} vs {K}")
    wt = None
    if x.dtype == F32:
        # fp32 build: one plain GEMM kernel for every shape (any M / N / K / strides), the preceding RMSNorm as its own launch; its output
        # is fp32 anyway and its epilogue rounds nothing
        route, rms_first = "f32", True
        out_f32 = bias_after_rounding = False
    else:
        route, rms_first = _linear_route(M, N, K, w.route_pitch if wq else w.stride(0), tune, w.fmt_name if wq else None, act_quant)
        if act_quant is not None and route in A8_ROUTES:
            for name, given in (("bias", bias is not None), ("act", act), ("bias_after_rounding", bias_after_rounding), ("tune", tune)):
                if given:
                    raise RuntimeError(f"u-llava_amd.linear: `{name}` is not supported on the activation-quantized route {route!r}")
            return _linear_a8(route, x, w, residual, swiglu, out, out_f32, rms_w, rms_eps)
        if wq and route == "gemm":
            # prefill shapes: dequantize into the stream's scratch, then the bf16 flow on dequant(w)
            w, wt = _wq_dequant_for_gemm(w, M)
            route, rms_first = _linear_route(M, N, K, w.stride(0), tune)
    if rms_w is not None and rms_first:
        x = rmsnorm(x, rms_w, rms_eps)
        rms_w = None
        M, ldx = _rows(x)
    out, flags, ldr = _epilogue(x, N, swiglu, out_f32, residual, out)
    flags |= ACTS[act] | (EPI_BIAS_ROUNDED if bias_after_rounding else 0)
    if bias is not None:
        _chk(bias, "bias", x.dtype)
        flags |= EPI_BIAS
    ldc = _rows(out)[1]
    st = _stream()
    if route == "f32":
        _lib.call("ull_gemm_f32", _p(x), ldx, _p(w), w.stride(0), _p(out), ldc, _p(bias), _p(residual), ldr, M, N, K, flags, None, 0, st)
    elif route == "gemm":
        if K % 64:
            # The MFMA kernel consumes K in 64-wide DMA tiles.  Every real width on the path (1024, 1280, 4096, 5120,
            # 11008, 256, 128, 2048, 64, patch K padded by im2col) is a multiple of 64; only the tiny test models are not.
            # Zero-padding K is exact (adds 0*0 terms).
            Kp = ((K + 63) // 64) * 64
            x = torch.nn.functional.pad(x.reshape(M, K) if x.dim() != 2 else x, (0, Kp - K))
            w = torch.nn.functional.pad(w, (0, Kp - K))
            K, ldx = Kp, Kp
        big = _big(M, N, K)
        if big and wt is None:
            wt = _tiled_of(w)
        ws_ptr, ws_bytes = _gemm_ws(x.device, st, big, M, N, K, small_m=True)
        wp, ldw, flags = (wt, K, flags | EPI_W_TILED) if wt is not None else (w, w.stride(0), flags)
        _lib.call("ull_gemm_" + _SFX[x.dtype], _p(x), ldx, _p(wp), ldw, _p(out), ldc, _p(bias), _p(residual), ldr, M, N, K, flags | tune,
                  ws_ptr, ws_bytes, st)
    else:
        sfx, wargs = _weight_args(w)
        if route == "skinny":
            _lib.call("ull_gemm_skinny_" + sfx, _p(x), ldx, *wargs, _p(out), ldc, _p(bias), _p(residual), ldr, M, N, K, flags, st)
        elif rms_w is not None:
            _chk(rms_w, "rms_w", x.dtype)
            _lib.call("ull_gemv_rmsnorm_" + sfx, _p(x), ldx, _p(rms_w), float(rms_eps), *wargs, _p(out), ldc, _p(bias), _p(residual), ldr, M, N, K,
                      flags, st)
        else:
            _lib.call("ull_gemv_" + sfx, _p(x), ldx, *wargs, _p(out), ldc, _p(bias), _p(residual), ldr, M, N, K, flags, st)
    return out


# ---- quantized activations on quantized weights (quantize_weights(activations=, activation_scope=)) ---------------------------------------
# Which Linear takes which kernel is `_linear_route`'s decision alone; `linear(..., act_quant=)` carries it out (`_linear_a8`) through the
# per-kernel wrappers linear_a8w8 / linear_w4a8 / linear_w4a4 / linear_a8w8_skinny / linear_w4a8_skinny, each the only call site of its entry.
A8_ROUTES = ("a8w8", "w4a8", "a8w8_skinny", "w4a4", "w4a8_skinny")


def _linear_a8(route: str, x, w, residual, swiglu: bool, out, out_f32: bool, rms_w, rms_eps: float) -> torch.Tensor:
    """`linear` on an A8 route: the RMSNorm rides in the row quantization ("a8w8_skinny", "w4a8_skinny") or is a launch of its own, then the
    route's wrapper."""
    kw = dict(residual=residual, swiglu=swiglu, out=out, out_f32=out_f32)
    if route in ("a8w8_skinny", "w4a8_skinny"):
        if route == "a8w8_skinny":
            xq, xs = quantize_rows_fp8(x) if rms_w is None else rmsnorm_quantize_rows_fp8(x, rms_w, rms_eps)
            y = linear_a8w8_skinny(xq, xs, w, **kw)
        else:
            xq, xs = _quantize_rows_mxfp8(x, x.shape[-1]) if rms_w is None else rmsnorm_quantize_rows_mxfp8(x, rms_w, rms_eps)
            y = linear_w4a8_skinny(xq, xs, w, **kw)
        return y if x.dim() == 2 or out is not None else y.view(*x.shape[:-1], y.shape[-1])
    if rms_w is not None:
        x = rmsnorm(x, rms_w, rms_eps)
    return {"a8w8": linear_a8w8, "w4a8": linear_w4a8, "w4a4": linear_w4a4}[route](x, w, **kw)


# ---- FP8 activations on FP8 weights: route "a8w8" ---------------------------------------------------------------------------------------
def quantize_rows_fp8(x: torch.Tensor):
    """(codes uint8 [M, K], scales fp32 [M]) of bf16 rows x [..., K] (one row pitch): quantize_fp8's rule per row, so every token gets its own
    power-of-two scale 2^t, t the smallest integer with amax|row| * 2^-t <= 448 (0 for an all-zero row); codes = e4m3fn(x * 2^-t), nearest even."""
    _chk(x, "x", BF16)
    M, ldx = _rows(x)
    K = x.shape[-1]
    codes = torch.empty(M, K, device=x.device, dtype=torch.uint8)
    scales = torch.empty(M, device=x.device, dtype=F32)
    _lib.call("ull_quantize_rows_fp8_bf16", _p(x), ldx, M, K, _p(codes), _p(scales), _stream())
    return codes, scales


def linear_a8w8(x: torch.Tensor, w: "Fp8Weight", residual: Optional[torch.Tensor] = None, swiglu: bool = False,
                out: Optional[torch.Tensor] = None, out_f32: bool = False) -> torch.Tensor:
    """y = epilogue(x @ w.T) with e4m3 activations on e4m3 weights (ull_gemm_a8w8_bf16; the only call site of that entry):
        xq, 2^t_m = quantize_rows_fp8(x)                        per token
        acc[m, n] = sum_k float(xq[m, k]) * float(wq[n, k])     exact products, fp32 accumulation in the kernel's fixed K order
        y[m, n]   = acc[m, n] * 2^(t_m + s_n)                   exact
    then `linear`'s epilogue on y (residual / swiglu / out_f32, same rounding points).  A K that is no multiple of 128 (tiny test models) is
    padded with zero codes, which adds 0 * 0 terms; the padded weight codes are kept on the Fp8Weight."""
    if not isinstance(w, Fp8Weight):
        raise RuntimeError("u-llava_amd.linear_a8w8: w must be an Fp8Weight")
    _chk(x, "x", BF16)
    M, _ = _rows(x)
    N, K = w.shape
    if x.shape[-1] != K:
        raise RuntimeError(f"u-llava_amd.linear_a8w8: K mismatch {x.shape[-1]} vs {K}")
    xq, xs = quantize_rows_fp8(x)
    wq = w.a8_codes()
    if wq is not w.codes:
        xq = torch.nn.functional.pad(xq, (0, -K % A8W8_BK))
    out, flags, ldr = _epilogue(x, N, swiglu, out_f32, residual, out, BF16)
    _lib.call("ull_gemm_a8w8_bf16", _p(xq), xq.stride(0), _p(xs), _p(wq), wq.stride(0), _p(w.scales), _p(out), _rows(out)[1], _p(residual), ldr,
              M, N, xq.shape[1], flags, _stream())
    return out


# ---- FP8 Linears of the SAM image encoder (SamEngine.linear_precision = "fp8_e4m3") -----------------------------------------------------
# Not a route of `linear`: the SAM block loop calls these two directly, at any M (the 128-tile kernel handles M < 128).
def layernorm_quantize_rows_fp8(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float):
    """quantize_rows_fp8(layernorm(x, w, b, eps)) in one launch (ull_layernorm_quantize_rows_fp8_bf16), bit for bit: (codes uint8 [M, K], scales
    fp32 [M]) of the normed bf16 rows, which are never written."""
    _chk(x, "x", BF16); _chk(w, "w", BF16); _chk(b, "b", BF16)
    M, ldx = _rows(x)
    K = x.shape[-1]
    codes = torch.empty(M, K, device=x.device, dtype=torch.uint8)
    scales = torch.empty(M, device=x.device, dtype=F32)
    _lib.call("ull_layernorm_quantize_rows_fp8_bf16", _p(x), ldx, _p(w), _p(b), float(eps), M, K, _p(codes), K, _p(scales), _stream())
    return codes, scales


def linear_a8w8_rows(xq: torch.Tensor, xs: torch.Tensor, w: "Fp8Weight", bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
                     residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_f32: bool = False) -> torch.Tensor:
    """y = epilogue(dequant(xq, xs) @ w.T) from activation codes xq uint8 [M, K] (rows contiguous) and their scales xs fp32 [M]
    (quantize_rows_fp8 / layernorm_quantize_rows_fp8) on an Fp8Weight, any M (ull_gemm_a8w8_epi_bf16; the only call site of that entry):
    linear_a8w8's arithmetic, then `linear`'s epilogue with its rounding points -- bf16 bias added to the fp32 sum, activation, residual,
    out_f32.  A K that is no multiple of 128 (tiny test models) is padded with zero codes, as linear_a8w8 does."""
    if not isinstance(w, Fp8Weight):
        raise RuntimeError("u-llava_amd.linear_a8w8_rows: w must be an Fp8Weight")
    if xq.dtype != torch.uint8 or xq.dim() != 2 or xq.stride(1) != 1 or xs.dtype != F32 or xs.shape != (xq.shape[0],) or not xs.is_contiguous():
        raise RuntimeError("u-llava_amd.linear_a8w8_rows: xq uint8 [M, K] (rows contiguous), xs fp32 [M]")
    M, K = xq.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise RuntimeError(f"u-llava_amd.linear_a8w8_rows: K mismatch {K} vs {w.shape[1]}")
    wq = w.a8_codes()
    if wq.shape[1] != K or xq.stride(0) % 16 or xq.data_ptr() % 16:
        xq = torch.nn.functional.pad(xq, (0, wq.shape[1] - K)).contiguous()
    out, flags, ldr = _epilogue(xq, N, False, out_f32, residual, out, BF16)
    flags |= ACTS[act]
    if bias is not None:
        _chk(bias, "bias", BF16)
        flags |= EPI_BIAS
    _lib.call("ull_gemm_a8w8_epi_bf16", _p(xq), xq.stride(0), _p(xs), _p(wq), wq.stride(0), _p(w.scales), _p(bias), _p(out), _rows(out)[1],
              _p(residual), ldr, M, N, xq.shape[1], flags, _stream())
    return out


# ---- FP8 activations on FP8 weights at decode shapes: route "a8w8_skinny" -------------------------------------------------------------
def rmsnorm_quantize_rows_fp8(x: torch.Tensor, w: torch.Tensor, eps: float):
    """quantize_rows_fp8(rmsnorm(x, w, eps)) in one launch (ull_rmsnorm_quantize_rows_fp8_bf16), bit for bit: (codes uint8 [M, K], scales
    fp32 [M]) of the normed bf16 rows, which are never written."""
    _chk(x, "x", BF16); _chk(w, "w", BF16)
    M, ldx = _rows(x)
    K = x.shape[-1]
    codes = torch.empty(M, K, device=x.device, dtype=torch.uint8)
    scales = torch.empty(M, device=x.device, dtype=F32)
    _lib.call("ull_rmsnorm_quantize_rows_fp8_bf16", _p(x), ldx, _p(w), float(eps), M, K, _p(codes), K, _p(scales), _stream())
    return codes, scales


def linear_a8w8_skinny(xq: torch.Tensor, xs: torch.Tensor, w: "Fp8Weight", residual: Optional[torch.Tensor] = None, swiglu: bool = False,
                       out: Optional[torch.Tensor] = None, out_f32: bool = False) -> torch.Tensor:
    """y = epilogue(dequant(xq, xs) @ w.T) at M <= 32 rows from activation codes xq uint8 [M, K] (rows contiguous, pitch a multiple of 16) and
    their scales xs fp32 [M] (quantize_rows_fp8 / rmsnorm_quantize_rows_fp8), on the weight-streaming W8A8 kernel (ull_gemm_skinny_a8w8_bf16;
    the only call site of that entry): linear_a8w8's arithmetic with a summation order that depends on K alone, then `linear`'s skinny
    epilogue (residual / swiglu / out_f32, same rounding points).  K % 128 == 0."""
    if not isinstance(w, Fp8Weight):
        raise RuntimeError("u-llava_amd.linear_a8w8_skinny: w must be an Fp8Weight")
    if xq.dtype != torch.uint8 or xq.dim() != 2 or xq.stride(1) != 1 or xs.dtype != F32 or xs.shape != (xq.shape[0],) or not xs.is_contiguous():
        raise RuntimeError("u-llava_amd.linear_a8w8_skinny: xq uint8 [M, K] (rows contiguous), xs fp32 [M]")
    M, K = xq.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise RuntimeError(f"u-llava_amd.linear_a8w8_skinny: K mismatch {K} vs {w.shape[1]}")
    wq = w.a8_codes()                                    # (aligned rows; a K that is no multiple of 128 is still the entry's to refuse)
    out, flags, ldr = _epilogue(xq, N, swiglu, out_f32, residual, out, BF16)
    _lib.call("ull_gemm_skinny_a8w8_bf16", _p(xq), xq.stride(0), _p(xs), _p(wq), wq.stride(0), _p(w.scales), _p(out), _rows(out)[1],
              _p(residual), ldr, M, N, K, flags, _stream())
    return out


# ---- MXFP8 activations on MXFP4 weights: route "w4a8" -----------------------------------------------------------------------------------
def w4a8_k_ok(K: int) -> bool:
    """Whether ull_gemm_w4a8_bf16 takes a weight of this K (K % 32 == 0): a multiple of its 128-code K-tile, or a K that padding brings there
    without creating a superblock (the resident layout of a padded row must stay the standard order: K < 2048 before and after)."""
    return K % A8W8_BK == 0 or K + (-K % A8W8_BK) < 2048


def _mxfp4_kpadded(w: "Mxfp4Weight", Kp: int):
    """(codes, scales) of w for a GEMM that walks Kp >= K in 128-code K-tiles: w's own, or -- K < 2048, tiny test models only -- the copy
    padded with zero codes and the scale byte 127, made once and kept on the weight (linear_w4a8 and linear_w4a4 share it)."""
    N, K = w.shape
    if Kp == K:
        return w.codes, w.scales
    if w._kpad is None:                      # K < 2048: the row is in standard order, so padding appends
        pc = torch.nn.functional.pad(w.codes, (0, (Kp - K) // 2)).contiguous()
        ps = torch.full((N, Mxfp4Weight.scale_pitch(Kp)), 127, device=w.codes.device, dtype=torch.uint8)
        ps[:, :K // 32] = w.scales[:, :K // 32]
        w._kpad = (pc, ps)
    return w._kpad


def _quantize_rows_mxfp8(x: torch.Tensor, Kp: int):
    """(codes uint8 [M, Kp], scale bytes uint8 [M, Mxfp4Weight.scale_pitch(Kp)]) as ull_gemm_w4a8_bf16 reads them: the scale byte of block j
    sits where the resident MXFP4 layout puts a weight's (`_mx_perm`); columns past K are zero codes, and every scale byte that belongs to
    no block of x (padding blocks, spare bytes of the pitch) is 127 (2^0)."""
    _chk(x, "x", BF16)
    M, ldx = _rows(x)
    K = x.shape[-1]
    if K % 32:
        raise RuntimeError(f"u-llava_amd.quantize_rows_mxfp8: K must be a multiple of 32, got {K}")
    lds = Mxfp4Weight.scale_pitch(Kp)
    codes = (torch.empty if Kp == K else torch.zeros)(M, Kp, device=x.device, dtype=torch.uint8)
    if lds == K // 32:
        scales = torch.empty(M, lds, device=x.device, dtype=torch.uint8)
    else:
        scales = torch.full((M, lds), 127, device=x.device, dtype=torch.uint8)
    _lib.call("ull_quantize_rows_mxfp8_bf16", _p(x), ldx, M, K, _p(codes), Kp, _p(scales), lds, _stream())
    return codes, scales


def quantize_rows_mxfp8(x: torch.Tensor):
    """(codes uint8 [M, K], scales uint8 [M, K / 32]) of bf16 rows x [..., K] (one row pitch, K % 32 == 0) in OCP MXFP8: per row and block of
    32 consecutive K elements the E8M0 byte t + 127, t the smallest integer with amax|block| * 2^-t <= 448 (0 for an all-zero block), clamped
    to [-127, 127]; codes = e4m3fn(x * 2^-t), nearest even -- bit-identical to torch's CPU cast `(x.float() * 2**-t).to(torch.float8_e4m3fn)`.
    The scales come back in block order; the W4A8 GEMM reads them in a private order (`_quantize_rows_mxfp8`)."""
    K = x.shape[-1]
    codes, raw = _quantize_rows_mxfp8(x, K)
    return codes, raw[:, _mx_perm(K, x.device)[1]]


def linear_w4a8(x: torch.Tensor, w: "Mxfp4Weight", residual: Optional[torch.Tensor] = None, swiglu: bool = False,
                out: Optional[torch.Tensor] = None, out_f32: bool = False) -> torch.Tensor:
    """y = epilogue(x @ w.T) with MXFP8 activations on the resident MXFP4 weight (ull_gemm_w4a8_bf16; the only call site of that entry):
        xq, t = quantize_rows_mxfp8(x)                                         per row and block j of 32 K elements
        y[m, n] = sum_j 2^(t[m, j] + s[n, j]) * sum_{k in j} float(xq[m, k]) * e2m1(wq[n, k])     exact products, scales applied by the
                                                                               instruction, fp32 accumulation in the kernel's fixed K order
    then `linear`'s epilogue on y (residual / swiglu / out_f32, same rounding points).  A K below 2048 that is no multiple of 128 (tiny test
    models) is padded with zero codes and the scale byte 127 on both sides, which adds 0 * 0 terms; the padded weight is kept on the
    Mxfp4Weight."""
    if not isinstance(w, Mxfp4Weight):
        raise RuntimeError("u-llava_amd.linear_w4a8: w must be an Mxfp4Weight")
    _chk(x, "x", BF16)
    M, _ = _rows(x)
    N, K = w.shape
    if x.shape[-1] != K:
        raise RuntimeError(f"u-llava_amd.linear_w4a8: K mismatch {x.shape[-1]} vs {K}")
    if not w4a8_k_ok(K):
        raise NotImplementedError(f"u-llava_amd.linear_w4a8: K = {K} is no multiple of 128 and cannot be padded (it would gain a superblock)")
    Kp = K + (-K % A8W8_BK)
    wq, wsc = _mxfp4_kpadded(w, Kp)
    xq, xsc = _quantize_rows_mxfp8(x, Kp)
    out, flags, ldr = _epilogue(x, N, swiglu, out_f32, residual, out, BF16)
    _lib.call("ull_gemm_w4a8_bf16", _p(xq), xq.stride(0), _p(xsc), xsc.stride(0), _p(wq), wq.stride(0), _p(wsc), wsc.stride(0), _p(out),
              _rows(out)[1], _p(residual), ldr, M, N, Kp, flags, _stream())
    return out


# ---- MXFP8 activations on MXFP4 weights at decode shapes: route "w4a8_skinny" -----------------------------------------------------------
def rmsnorm_quantize_rows_mxfp8(x: torch.Tensor, w: torch.Tensor, eps: float):
    """_quantize_rows_mxfp8(rmsnorm(x, w, eps), K) in one launch (ull_rmsnorm_quantize_rows_mxfp8_bf16), bit for bit: (codes uint8 [M, K], scale
    bytes uint8 [M, Mxfp4Weight.scale_pitch(K)] in the order the W4A8 kernels read) of the normed bf16 rows, which are never written.
    K % 32 == 0; scale bytes that belong to no block (spare bytes of the pitch) are 127."""
    _chk(x, "x", BF16); _chk(w, "w", BF16)
    M, ldx = _rows(x)
    K = x.shape[-1]
    if K % 32:
        raise RuntimeError(f"u-llava_amd.rmsnorm_quantize_rows_mxfp8: K must be a multiple of 32, got {K}")
    lds = Mxfp4Weight.scale_pitch(K)
    codes = torch.empty(M, K, device=x.device, dtype=torch.uint8)
    if lds == K // 32:
        scales = torch.empty(M, lds, device=x.device, dtype=torch.uint8)
    else:
        scales = torch.full((M, lds), 127, device=x.device, dtype=torch.uint8)
    _lib.call("ull_rmsnorm_quantize_rows_mxfp8_bf16", _p(x), ldx, _p(w), float(eps), M, K, _p(codes), K, _p(scales), lds, _stream())
    return codes, scales


def linear_w4a8_skinny(xq: torch.Tensor, xsc: torch.Tensor, w: "Mxfp4Weight", residual: Optional[torch.Tensor] = None, swiglu: bool = False,
                       out: Optional[torch.Tensor] = None, out_f32: bool = False) -> torch.Tensor:
    """y = epilogue(dequant(xq, xsc) @ w.T) at M <= 32 rows from MXFP8 activation codes xq uint8 [M, K] (rows contiguous, pitch a multiple of 16)
    and their scale bytes xsc uint8 [M, >= K / 32] (`_quantize_rows_mxfp8` / rmsnorm_quantize_rows_mxfp8: the W4A8 pair's order), on the
    weight-streaming W4A8 kernel (ull_gemm_skinny_w4a8_bf16; the only call site of that entry): linear_w4a8's arithmetic from the resident
    MXFP4 codes and scale bytes with a summation order that depends on K alone, then `linear`'s skinny epilogue (residual / swiglu / out_f32,
    same rounding points).  K % 128 == 0 (a padded K is the entry's to refuse)."""
    if not isinstance(w, Mxfp4Weight):
        raise RuntimeError("u-llava_amd.linear_w4a8_skinny: w must be an Mxfp4Weight")
    if (xq.dtype != torch.uint8 or xq.dim() != 2 or xq.stride(1) != 1 or xsc.dtype != torch.uint8 or xsc.dim() != 2 or xsc.stride(1) != 1
            or xsc.shape[0] != xq.shape[0]):
        raise RuntimeError("u-llava_amd.linear_w4a8_skinny: xq uint8 [M, K] (rows contiguous), xsc uint8 [M, K / 32 or more] (rows contiguous)")
    M, K = xq.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise RuntimeError(f"u-llava_amd.linear_w4a8_skinny: K mismatch {K} vs {w.shape[1]}")
    out, flags, ldr = _epilogue(xq, N, swiglu, out_f32, residual, out, BF16)
    _lib.call("ull_gemm_skinny_w4a8_bf16", _p(xq), xq.stride(0), _p(xsc), xsc.stride(0), _p(w.codes), w.codes.stride(0), _p(w.scales),
              w.scales.stride(0), _p(out), _rows(out)[1], _p(residual), ldr, M, N, K, flags, _stream())
    return out


# ---- MXFP4 activations on MXFP4 weights: route "w4a4" -----------------------------------------------------------------------------------
def _quantize_rows_mxfp4(x: torch.Tensor, Kp: int, layout: int):
    """(codes uint8 [M, Kp / 2], scale bytes uint8 [M, Mxfp4Weight.scale_pitch(Kp)]) of ull_quantize_act_rows_mxfp4_bf16; layout 1: as
    ull_gemm_w4a4_bf16 reads them (private to that pair).  Columns past K are zero codes, and every scale byte that belongs to no block of x
    (padding blocks, spare bytes of the pitch) is 127 (2^0).  Kp != K only below 2048, where layout 1 stores the K-tiles in standard order."""
    _chk(x, "x", BF16)
    M, ldx = _rows(x)
    K = x.shape[-1]
    if K % 32:
        raise RuntimeError(f"u-llava_amd.quantize_rows_mxfp4: K must be a multiple of 32, got {K}")
    lds = Mxfp4Weight.scale_pitch(Kp)
    codes = (torch.empty if Kp == K else torch.zeros)(M, Kp // 2, device=x.device, dtype=torch.uint8)
    if lds == K // 32:
        scales = torch.empty(M, lds, device=x.device, dtype=torch.uint8)
    else:
        scales = torch.full((M, lds), 127, device=x.device, dtype=torch.uint8)
    _lib.call("ull_quantize_act_rows_mxfp4_bf16", _p(x), ldx, M, K, _p(codes), Kp // 2, _p(scales), lds, layout, _stream())
    return codes, scales


def quantize_rows_mxfp4(x: torch.Tensor):
    """(codes uint8 [M, K / 2], scales uint8 [M, K / 32]) of bf16 rows x [..., K] (one row pitch, K % 32 == 0) in OCP MXFP4, the weights' rule
    per row and block of 32 consecutive K elements: the E8M0 byte t + 127, t the smallest integer with amax|block| * 2^-t <= 6 (0 for an
    all-zero block), clamped to [-125, 126]; codes = e2m1(x * 2^-t), nearest, ties to the even code -- bit for bit
    `quantize_mxfp4(x).to_standard()`.  Standard layout (element 2i in the low nibble of byte i, scales in block order); the W4A4 GEMM reads
    a private order (`_quantize_rows_mxfp4(x, K, 1)`)."""
    K = x.shape[-1]
    codes, raw = _quantize_rows_mxfp4(x, K, 0)
    return codes, raw[:, :K // 32]


def linear_w4a4(x: torch.Tensor, w: "Mxfp4Weight", residual: Optional[torch.Tensor] = None, swiglu: bool = False,
                out: Optional[torch.Tensor] = None, out_f32: bool = False) -> torch.Tensor:
    """y = epilogue(x @ w.T) with MXFP4 activations on the resident MXFP4 weight (ull_gemm_w4a4_bf16; the only call site of that entry):
        xq, t = quantize_rows_mxfp4(x)                                         per row and block j of 32 K elements
        y[m, n] = sum_j 2^(t[m, j] + s[n, j]) * sum_{k in j} e2m1(xq[m, k]) * e2m1(wq[n, k])      exact products, scales applied by the
                                                                               instruction, fp32 accumulation in the kernel's fixed K order
    then `linear`'s epilogue on y (residual / swiglu / out_f32, same rounding points).  A K below 2048 that is no multiple of 128 (tiny test
    models) is padded with zero codes and the scale byte 127 on both sides, which adds 0 * 0 terms; the padded weight is the one linear_w4a8
    keeps on the Mxfp4Weight."""
    if not isinstance(w, Mxfp4Weight):
        raise RuntimeError("u-llava_amd.linear_w4a4: w must be an Mxfp4Weight")
    _chk(x, "x", BF16)
    M, _ = _rows(x)
    N, K = w.shape
    if x.shape[-1] != K:
        raise RuntimeError(f"u-llava_amd.linear_w4a4: K mismatch {x.shape[-1]} vs {K}")
    if not w4a8_k_ok(K):
        raise NotImplementedError(f"u-llava_amd.linear_w4a4: K = {K} is no multiple of 128 and cannot be padded (it would gain a superblock)")
    Kp = K + (-K % A8W8_BK)
    wq, wsc = _mxfp4_kpadded(w, Kp)
    xq, xsc = _quantize_rows_mxfp4(x, Kp, 1)
    out, flags, ldr = _epilogue(x, N, swiglu, out_f32, residual, out, BF16)
    _lib.call("ull_gemm_w4a4_bf16", _p(xq), xq.stride(0), _p(xsc), xsc.stride(0), _p(wq), wq.stride(0), _p(wsc), wsc.stride(0), _p(out),
              _rows(out)[1], _p(residual), ldr, M, N, Kp, flags, _stream())
    return out


def rope_table(positions: torch.Tensor, inv_freq: torch.Tensor, dtype) -> tuple:
    """(cos, sin) [tokens, hd/2] of `dtype` for int64 positions [tokens]: LlamaRotaryEmbedding's fp32 cos / sin cast to the model dtype."""
    _chk(positions, "positions", torch.int64); _chk(inv_freq, "inv_freq", torch.float32)
    if dtype not in _SFX:
        raise RuntimeError("u-llava_amd.rope_table: dtype must be bf16 or fp16")
    T, half = positions.numel(), inv_freq.numel()
    cs = torch.empty(T, half, device=positions.device, dtype=dtype)
    sn = torch.empty(T, half, device=positions.device, dtype=dtype)
    _lib.call("ull_rope_table_" + _SFX[dtype], _p(positions), _p(inv_freq), T, half, _p(cs), _p(sn), _stream())
    return cs, sn


GEMM_TUNE_WAVES8, GEMM_TUNE_WAVES4 = _D["ULL_GEMM_TUNE_WAVES8"], _D["ULL_GEMM_TUNE_WAVES4"]     # force one form of the 256x256 kernel (tests / tools)


def linear_qkv_rope(x: torch.Tensor, w: torch.Tensor, rope_cos: torch.Tensor, rope_sin: torch.Tensor, rope_cols: int, head_dim: int,
                    out: Optional[torch.Tensor] = None, tune: int = 0) -> torch.Tensor:
    """Fused q|k|v projection + RoPE on the first `rope_cols` output columns (q and k heads), head_dim 128, K % 64 == 0, M > 4.
    Bit-identical to linear() followed by rope_inplace().  w may be an `Fp8Weight` / `Mxfp4Weight` (dequantized into a scratch first)."""
    wt = None
    if isinstance(w, QuantWeight):
        if x.dtype != BF16:
            raise RuntimeError(f"u-llava_amd.linear_qkv_rope: {w.fmt_name} weights need bf16 activations, got {x.dtype}")
        w, wt = _wq_dequant_for_gemm(w, _rows(x)[0])
    _chk(x, "x"); _chk(w, "w", x.dtype); _chk(rope_cos, "rope_cos", x.dtype); _chk(rope_sin, "rope_sin", x.dtype)
    M, ldx = _rows(x)
    N, K = w.shape
    if x.shape[-1] != K or K % 64 or head_dim != 128 or rope_cos.shape != (M, 64) or not rope_cos.is_contiguous() or not rope_sin.is_contiguous():
        raise RuntimeError("u-llava_amd.linear_qkv_rope: needs K % 64 == 0, head_dim == 128 and [M, 64] contiguous tables")
    if out is None:
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=x.dtype)
    _, ldc = _rows(out)
    big = _big(M, N, K)
    if big and wt is None:
        wt = _tiled_of(w)
    st = _stream()
    ws_ptr, ws_bytes = _gemm_ws(x.device, st, big, M, N, K, small_m=False)
    wp, ldw, flags = (wt, K, EPI_W_TILED) if wt is not None else (w, w.stride(0), 0)
    _lib.call("ull_gemm_qkv_rope_" + _SFX[x.dtype], _p(x), ldx, _p(wp), ldw, _p(out), ldc, M, N, K, _p(rope_cos), _p(rope_sin), rope_cols, head_dim,
              flags | tune, ws_ptr, ws_bytes, st)
    return out


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x, "x"); _chk(w, "w", x.dtype)
    rows, ldx = _rows(x)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    _, ldy = _rows(out)
    _lib.call("ull_rmsnorm_" + _SFX[x.dtype], _p(x), ldx, _p(w), _p(out), ldy, rows, x.shape[-1], float(eps), _stream())
    return out


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x, "x"); _chk(w, "w", x.dtype); _chk(b, "b", x.dtype)
    rows, ldx = _rows(x)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    _, ldy = _rows(out)
    _lib.call("ull_layernorm_" + _SFX[x.dtype], _p(x), ldx, _p(w), _p(b), _p(out), ldy, rows, x.shape[-1], float(eps), _stream())
    return out


def clip_embed_ln(patch: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, w: torch.Tensor, b: torch.Tensor, n_img: int, tokens: int,
                  eps: float) -> torch.Tensor:
    """patch [n_img*(tokens-1), D] -> pre-LN hidden states [n_img, tokens, D]."""
    _chk(patch, "patch")
    for t, n in ((cls, "cls"), (pos, "pos"), (w, "w"), (b, "b")):
        _chk(t, n, patch.dtype)
    D = patch.shape[-1]
    out = torch.empty(n_img, tokens, D, device=patch.device, dtype=patch.dtype)
    _lib.call("ull_clip_embed_ln_" + _SFX[patch.dtype], _p(patch), patch.stride(0), _p(cls), _p(pos), _p(w), _p(b), _p(out), D, n_img, tokens, D,
              float(eps), _stream())
    return out


_REL_POS_CACHE: dict = {}          # id(table) -> (weakref(table), version, n, resized): only the very same tensor object may hit


def fit_rel_pos(rel_pos: torch.Tensor, size: int) -> torch.Tensor:
    """get_rel_pos's resize (image_encoder.py:333-345): a table whose length is not 2 * size - 1 is linearly interpolated to that length.
    The resized copy is kept for the tensor OBJECT it was made from (a module parameter), never by address: a temporary's storage
    is reused by the allocator."""
    n = 2 * size - 1
    if rel_pos.shape[0] == n:
        return rel_pos
    _chk(rel_pos, "rel_pos")
    hit = _REL_POS_CACHE.get(id(rel_pos))
    if hit is not None and hit[0]() is rel_pos and hit[1] == rel_pos._version and hit[2] == n:
        return hit[3]
    out = torch.empty(n, rel_pos.shape[1], device=rel_pos.device, dtype=rel_pos.dtype)
    _lib.call("ull_interp_rows_linear_" + _SFX[rel_pos.dtype], _p(rel_pos.contiguous()), _p(out), rel_pos.shape[0], n, rel_pos.shape[1], _stream())
    for k in [k for k, v in _REL_POS_CACHE.items() if v[0]() is None]:
        del _REL_POS_CACHE[k]
    _REL_POS_CACHE[id(rel_pos)] = (weakref.ref(rel_pos), rel_pos._version, n, out)
    return out


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, B: int, H: int, Sq: int, Sk: int, hd: int,
              q_strides, k_strides, o_strides, key_mask: Optional[torch.Tensor] = None, causal: bool = False, scale_mode: int = 1,
              scale: float = 1.0, q_scale: float = 1.0, rel_h: Optional[torch.Tensor] = None, rel_w: Optional[torch.Tensor] = None,
              rel_pos_hw: Optional[tuple] = None, v_strides=None):
    """rel_h/rel_w: either per-query bias tables [B*H, Sq, KH|KW] (from sam_relpos), or -- with rel_pos_hw=(KH, KW) -- the raw
    rel_pos_h / rel_pos_w parameters [2KH-1, hd] / [2KW-1, hd], in which case the kernel builds the tables itself.
    v_strides = (batch, head, token) strides: `vt` is V ITSELF ([B,H,Sk,hd] by strides), not its transposed image; the kernels that
    transpose on the fly (LLaMA / CLIP prefill) take it directly, for any other shape the V^T image is made here first."""
    _chk(q, "q"); _chk(k, "k", q.dtype); _chk(vt, "vt", q.dtype); _chk(out, "out", q.dtype)
    rel_mode, kh, kw = 0, 0, 0
    if rel_h is not None and rel_pos_hw is not None and q.dtype == F32:
        # fp32 build: the per-query bias tables come from their own kernel (rel_mode 1); the 16-bit kernels build them in place (rel_mode 2)
        kh, kw = rel_pos_hw
        rel_h, rel_w = sam_relpos(q, q_strides, fit_rel_pos(rel_h, kh), fit_rel_pos(rel_w, kw), B, H, kh, kw, hd)
        rel_pos_hw = None
    if rel_h is not None:
        _chk(rel_h, "rel_h", q.dtype); _chk(rel_w, "rel_w", q.dtype)
        if rel_pos_hw is not None:
            rel_mode, (kh, kw) = 2, rel_pos_hw
            rel_h, rel_w = fit_rel_pos(rel_h, kh), fit_rel_pos(rel_w, kw)
            if rel_h.shape[1] != hd or rel_w.shape[1] != hd:
                raise ValueError(f"rel_pos tables of width {rel_h.shape[1]} / {rel_w.shape[1]} for head_dim {hd}")
        else:
            rel_mode, kh, kw = 1, rel_h.shape[-1], rel_w.shape[-1]
    if key_mask is not None:
        _chk(key_mask, "key_mask", torch.int32)
    name = "ull_attention_" + _SFX[q.dtype]
    tail = (_p(out), *o_strides, _p(key_mask), B, H, Sq, Sk, hd, int(causal), scale_mode, float(scale), float(q_scale), _p(rel_h), _p(rel_w),
            kh, kw, rel_mode, _zeros(q.device).data_ptr(), _stream())
    if v_strides is not None:
        rc = _lib.query(name, _p(q), *q_strides, _p(k), *k_strides, _p(vt), *v_strides, 0, *tail)
        if rc == 0:
            return out
        if rc != -2:                               # anything but "no kernel of that form for this shape"
            raise RuntimeError(f"u-llava_amd: {name} failed: {_lib.ERRORS.get(rc, rc)}")
        if v_strides[1] != hd:
            raise ValueError("V rows must have their heads contiguous (head stride == head_dim) to be transposed here")
        vt = transpose_v(vt, v_strides[0], v_strides[2], B, Sk, H, hd)
    pitch = vt.shape[-1]
    _lib.call(name, _p(q), *q_strides, _p(k), *k_strides, _p(vt), H * hd * pitch, hd * pitch, pitch, pitch, *tail)
    return out


def quantize_kv(k: torch.Tensor, k_strides, v: torch.Tensor, v_strides, k8: torch.Tensor, vt8: torch.Tensor, k_scale: torch.Tensor,
                vt_scale: torch.Tensor, p0: int, n: int, src_p0: int = 0, v_image: bool = False) -> None:
    """Positions p0 .. p0 + n - 1 of one layer's fp8 KV cache (codes k8 [B, H, smax, hd] / vt8 [B, H, hd, smax], scales [B, H, smax]) from
    bf16 K rows (k_strides = batch, head, position) and V rows (v_strides likewise) or, with v_image, a V^T image in the permuted slot order
    (v_strides = batch, head, d); source position src_p0 + s.  Codes and scales follow the fp8-weight rule (bit-identical to torch's cast)."""
    _chk(k, "k", BF16); _chk(v, "v", BF16)
    B, H, smax, hd = k8.shape
    _lib.call("ull_kv8_quantize_bf16", _p(k), *k_strides, _p(v), *v_strides, int(v_image), src_p0, _p(k8), _p(vt8), _p(k_scale), _p(vt_scale),
              B, H, hd, smax, p0, n, _stream())


def dequantize_kv(k8: torch.Tensor, vt8: torch.Tensor, k_scale: torch.Tensor, vt_scale: torch.Tensor, n: int, k_out: Optional[torch.Tensor] = None,
                  vt_out: Optional[torch.Tensor] = None) -> None:
    """Positions [0, n) of one layer's fp8 KV cache as bf16: k_out [B, H, P, hd] rows 0 .. n - 1, vt_out [B, H, hd, P'] (permuted V^T, slots up
    to round_up(n, 64), keys >= n zero).  Exactly the operands attention_kv8 reads."""
    B, H, smax, hd = k8.shape
    for t, nm, shp in ((k_out, "k_out", (B, H, None, hd)), (vt_out, "vt_out", (B, H, hd, None))):
        if t is not None:
            _chk(t, nm, BF16)
            if t.dim() != 4 or not t.is_contiguous() or any(a is not None and a != b for a, b in zip(shp, t.shape)):
                raise RuntimeError(f"u-llava_amd.dequantize_kv: {nm} must be a contiguous bf16 tensor of shape {shp}")
    _lib.call("ull_kv8_dequantize_bf16", _p(k8), _p(vt8), _p(k_scale), _p(vt_scale), B, H, hd, smax, n, _p(k_out),
              k_out.shape[2] if k_out is not None else 0, _p(vt_out), vt_out.shape[3] if vt_out is not None else 0, _stream())


def attention_kv8(q: torch.Tensor, q_strides, k_stage: torch.Tensor, vt_stage: torch.Tensor, k8: torch.Tensor, vt8: torch.Tensor,
                  k_scale: torch.Tensor, vt_scale: torch.Tensor, out: torch.Tensor, o_strides, B: int, H: int, Sq: int, Sk: int, hd: int,
                  key_mask: Optional[torch.Tensor], scale: float) -> torch.Tensor:
    """The LLaMA decode call of `attention` (causal, scale_mode 1) over an fp8 cache: keys < Sk - Sq from the codes, the Sq new keys from
    the staging window (k_stage [B, H, 128, hd], vt_stage [B, H, hd, 128], key k at row / slot k - w0, w0 = (Sk - Sq) rounded down to 64,
    where rope_append / linear_qkv_rope_append put them with smax = 128 and past - w0).  Stores the new keys' codes and scales.  Same bits
    as `attention` on the dequantized cache.  Sq <= 16 and 64 < Sk <= 4096."""
    _chk(q, "q", BF16); _chk(out, "out", BF16); _chk(k_stage, "k_stage", BF16); _chk(vt_stage, "vt_stage", BF16)
    if key_mask is not None:
        _chk(key_mask, "key_mask", torch.int32)
    if k_stage.shape != (B, H, 128, hd) or vt_stage.shape != (B, H, hd, 128) or k8.shape[:2] != (B, H) or k8.shape[3] != hd:
        raise RuntimeError("u-llava_amd.attention_kv8: staging / cache shapes")
    _lib.call("ull_attention_kv8_bf16", _p(q), *q_strides, _p(k_stage), _p(vt_stage), _p(k8), _p(vt8), _p(k_scale), _p(vt_scale), k8.shape[2],
              _p(out), *o_strides, _p(key_mask), B, H, Sq, Sk, hd, float(scale), _zeros(q.device).data_ptr(), _stream())
    return out


def dropout_apply(x: torch.Tensor, keep: torch.Tensor, p: float) -> torch.Tensor:
    """y = keep ? x / (1 - p) : 0 (keep: uint8, same number of elements)."""
    _chk(x, "x"); _chk(keep, "keep", torch.uint8)
    x = x.contiguous()
    y = torch.empty_like(x)
    _lib.call("ull_dropout_apply_" + _SFX[x.dtype], _p(x), _p(keep), _p(y), x.numel(), float(1.0 / (1.0 - p)), _stream())
    return y


def sam_window_attention(qkv: torch.Tensor, pad_row: torch.Tensor, rel_pos_h: torch.Tensor, rel_pos_w: torch.Tensor, B: int, H: int, W: int,
                         nH: int, hd: int, ws: int) -> torch.Tensor:
    """Block.forward's window_partition + Attention + window_unpartition (image_encoder.py:176-190) on image-order tokens:
    qkv [B*H*W, 3*nH*hd] -> [B*H*W, nH*hd].  pad_row: the qkv bias (= the q|k|v of a zero-padded token)."""
    _chk(qkv, "qkv"); _chk(pad_row, "pad_row", qkv.dtype); _chk(rel_pos_h, "rel_pos_h", qkv.dtype); _chk(rel_pos_w, "rel_pos_w", qkv.dtype)
    rel_pos_h, rel_pos_w = fit_rel_pos(rel_pos_h, ws), fit_rel_pos(rel_pos_w, ws)
    C = nH * hd
    if qkv.shape != (B * H * W, 3 * C) or pad_row.numel() != 3 * C:
        raise ValueError(f"qkv {tuple(qkv.shape)} / pad_row {tuple(pad_row.shape)} for B={B} H={H} W={W} C={C}")
    out = torch.empty(B * H * W, C, device=qkv.device, dtype=qkv.dtype)
    _lib.call("ull_sam_window_attention_" + _SFX[qkv.dtype], _p(qkv), 3 * C, _p(pad_row), _p(rel_pos_h), _p(rel_pos_w), _p(out), C,
              B, H, W, nH, hd, ws, float(hd ** -0.5), _zeros(qkv.device).data_ptr(), _stream())
    return out


def sam_global_exact_takes(side: int, hd: int, dtype) -> bool:
    """Whether `sam_global_attention_exact` has a kernel for a global block on a side x side grid: the ViT-H shape (64 x 64 tokens, head
    dim 80) in the two 16-bit builds.  (The fp32 build's attention already normalises before it rounds -- it rounds nothing.)"""
    return side == 64 and hd == 80 and dtype in (BF16, F16)


def sam_global_attention_exact(qkv: torch.Tensor, rel_pos_h: torch.Tensor, rel_pos_w: torch.Tensor, B: int, H: int, side: int, hd: int,
                               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention.forward of a SAM global block (image_encoder.py:196-260) with the reference's rounding point: softmax normalised in fp32,
    THEN rounded, then attn @ v (the default route, `attention` with rel_pos_hw, rounds exp(s - running max) and divides at the end).
    qkv [B * side * side, >= 3 * H * hd] rows q | k | v (any row pitch that is a multiple of 8) -> out [B * side * side, H * hd] (a view
    with a wider row pitch is fine).  Two passes over the keys in one launch; `sam_global_exact_takes` says which shapes have a kernel."""
    _chk(qkv, "qkv"); _chk(rel_pos_h, "rel_pos_h", qkv.dtype); _chk(rel_pos_w, "rel_pos_w", qkv.dtype)
    if not sam_global_exact_takes(side, hd, qkv.dtype):
        raise NotImplementedError(f"u-llava_amd: no exact SAM global-attention kernel for a {side} x {side} grid with head dim {hd} in {qkv.dtype}")
    S, C = side * side, H * hd
    if qkv.dim() != 2 or qkv.shape[0] != B * S or qkv.shape[1] < 3 * C:
        raise ValueError(f"qkv {tuple(qkv.shape)} for B={B} side={side} C={C}")
    rel_pos_h, rel_pos_w = fit_rel_pos(rel_pos_h, side), fit_rel_pos(rel_pos_w, side)
    if rel_pos_h.shape[1] != hd or rel_pos_w.shape[1] != hd:
        raise ValueError(f"rel_pos tables of width {rel_pos_h.shape[1]} / {rel_pos_w.shape[1]} for head_dim {hd}")
    if out is None:
        out = torch.empty(B * S, C, device=qkv.device, dtype=qkv.dtype)
    _chk(out, "out", qkv.dtype)
    if out.dim() != 2 or out.shape != (B * S, C):
        raise ValueError(f"out {tuple(out.shape)} for B={B} side={side} C={C}")
    ld, ldo = qkv.stride(0), out.stride(0)
    st = (S * ld, hd, ld)
    _lib.call("ull_sam_global_attention_exact_" + _SFX[qkv.dtype], _p(qkv), *st, _p(qkv[:, C:]), *st, _p(qkv[:, 2 * C:]), *st,
              _p(rel_pos_h.contiguous()), _p(rel_pos_w.contiguous()), B, H, side, hd, float(hd ** -0.5), _p(out), S * ldo, hd, ldo, _stream())
    return out


def rope_inplace(x: torch.Tensor, row_stride: int, positions: torch.Tensor, inv_freq: torch.Tensor, tokens: int, n_heads: int, hd: int):
    _chk(x, "x"); _chk(positions, "positions", torch.int64); _chk(inv_freq, "inv_freq", torch.float32)
    _lib.call("ull_rope_inplace_" + _SFX[x.dtype], _p(x), row_stride, _p(positions), _p(inv_freq), tokens, n_heads, hd, _stream())


def rope_append(qkv: torch.Tensor, row_stride: int, positions: torch.Tensor, inv_freq: torch.Tensor, B: int, S: int, H: int, hd: int,
                k_cache: torch.Tensor, vt_cache: torch.Tensor, smax: int, past: int):
    """decode step: RoPE on q (in place) and k + append of k / v to the KV cache (K [B,H,smax,hd], V^T [B,H,hd,smax] permuted)."""
    _chk(qkv, "qkv"); _chk(positions, "positions", torch.int64); _chk(inv_freq, "inv_freq", torch.float32)
    _chk(k_cache, "k_cache", qkv.dtype); _chk(vt_cache, "vt_cache", qkv.dtype)
    _lib.call("ull_rope_append_" + _SFX[qkv.dtype], _p(qkv), row_stride, _p(positions), _p(inv_freq), B, S, H, hd, _p(k_cache), _p(vt_cache), smax, past,
              _stream())


def linear_qkv_rope_append(x: torch.Tensor, w_qkv: torch.Tensor, rope_cos: torch.Tensor, rope_sin: torch.Tensor, B: int, S: int, H: int, hd: int,
                           k_cache: torch.Tensor, vt_cache: torch.Tensor, smax: int, past: int, rms_w: Optional[torch.Tensor] = None,
                           rms_eps: float = 0.0) -> torch.Tensor:
    """decode step (B * S <= 4 tokens): q | k | v projection of x (optionally RMS-normalised first) with RoPE and the KV-cache append in the
    GEMV's epilogue.  Returns the rotated queries [B * S, H * hd]; the rotated keys / the values land in the caches.  Same bits as
    `linear(x, w_qkv, rms_w=...)` followed by `rope_append`.  w_qkv may be an `Fp8Weight` / `Mxfp4Weight` (bf16 only)."""
    if not isinstance(w_qkv, QuantWeight):
        _chk(w_qkv, "w_qkv", x.dtype)
    elif x.dtype != BF16:
        raise RuntimeError(f"u-llava_amd.linear_qkv_rope_append: {w_qkv.fmt_name} weights need bf16 activations, got {x.dtype}")
    _chk(x, "x"); _chk(rope_cos, "rope_cos", x.dtype); _chk(rope_sin, "rope_sin", x.dtype)
    _chk(k_cache, "k_cache", x.dtype); _chk(vt_cache, "vt_cache", x.dtype)
    T, K = x.shape
    if T != B * S or T > 4 or w_qkv.shape != (3 * H * hd, K) or rope_cos.shape != (T, hd // 2) or rope_sin.shape != (T, hd // 2):
        raise RuntimeError("u-llava_amd.linear_qkv_rope_append: shapes (at most 4 tokens; w [3 * H * hd, K]; cos / sin [tokens, hd / 2])")
    if not (rope_cos.is_contiguous() and rope_sin.is_contiguous()):
        raise RuntimeError("u-llava_amd.linear_qkv_rope_append: rows must be contiguous")
    if rms_w is not None:
        _chk(rms_w, "rms_w", x.dtype)
    q = torch.empty(T, H * hd, device=x.device, dtype=x.dtype)
    sfx, wargs = _weight_args(w_qkv)
    _lib.call("ull_gemv_qkv_rope_append_" + sfx, _p(x), x.stride(0), _p(rms_w), float(rms_eps), *wargs, _p(q), q.stride(0), _p(rope_cos), _p(rope_sin),
              _p(k_cache), _p(vt_cache), B, S, H, hd, K, smax, past, _stream())
    return q


def transpose_v(v: torch.Tensor, v_bs: int, v_ss: int, B: int, S: int, H: int, hd: int, pitch: Optional[int] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(v, "v")
    pitch = pitch or ((S + 63) // 64) * 64
    vt = out if out is not None else torch.empty(B, H, hd, pitch, device=v.device, dtype=v.dtype)
    _lib.call("ull_transpose_v_" + _SFX[v.dtype], _p(v), v_bs, v_ss, _p(vt), B, S, H, hd, pitch, _stream())
    return vt


def im2col(img: torch.Tensor, ps: int, Kp: int) -> torch.Tensor:
    _chk(img, "img")
    if not img.is_contiguous():
        raise RuntimeError("u-llava_amd.im2col: image batch must be contiguous NCHW")
    n, C, H, W = img.shape
    out = torch.empty(n * (H // ps) * (W // ps), Kp, device=img.device, dtype=img.dtype)
    _lib.call("ull_im2col_" + _SFX[img.dtype], _p(img), _p(out), n, C, H, W, ps, Kp, _stream())
    return out


def pack_patch_weight(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [N, C, ps, ps] -> the [N, Kp] layout of ull_patchify_bf16: (c, ky) segments of 16 with kx >= ps zero, zero
    segments up to a multiple of 64."""
    N, C, ps, ps2 = w.shape
    if ps != ps2 or ps > 16 or ps % 2:
        raise NotImplementedError("patch sizes on the path: 14 (CLIP) and 16 (SAM)")
    K = C * ps * 16
    Kp = (K + 63) // 64 * 64
    out = torch.zeros(N, Kp, device=w.device, dtype=w.dtype)
    out[:, :K].view(N, C * ps, 16)[:, :, :ps] = w.reshape(N, C * ps, ps)
    return out


def patchify(img: torch.Tensor, wp: torch.Tensor, ps: int, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv2d(kernel = stride = ps) patch embedding straight from the pixels: img [n, C, H, W] bf16 -> [n*(H/ps)*(W/ps), N]."""
    _chk(img, "img"); _chk(wp, "packed patch weight", img.dtype)
    if not img.is_contiguous():
        raise RuntimeError("u-llava_amd.patchify: image batch must be contiguous NCHW")
    n, C, H, W = img.shape
    N, Kp = wp.shape
    out = torch.empty(n * (H // ps) * (W // ps), N, device=img.device, dtype=img.dtype)
    _lib.call("ull_patchify_" + _SFX[img.dtype], _p(img), n, C, H, W, ps, _p(wp), Kp, _p(bias), _p(out), N, N, _zeros(img.device).data_ptr(), _stream())
    return out


def mm_spans(ids: torch.Tensor, img_start: int, img_end: int, vid_start: int, vid_end: int, vocab: int = 0) -> torch.Tensor:
    """int32 [B, 4] = {kind, first start pos, feature index, error bits (1: start/end counts differ, 2: id outside [0, vocab))}."""
    _chk(ids, "input_ids", torch.int64)
    B, S = ids.shape
    spans = torch.empty(B, 4, device=ids.device, dtype=torch.int32)
    _lib.call("ull_mm_spans", _p(ids), B, S, img_start, img_end, vid_start, vid_end, vocab, _p(spans), _stream())
    return spans


def embed_splice(ids: torch.Tensor, table: torch.Tensor, img_feat: Optional[torch.Tensor], vid_feat: Optional[torch.Tensor],
                 spans: Optional[torch.Tensor], img_tokens: int = 0, img_pitch: int = 0, img_off: int = 0) -> torch.Tensor:
    """img_feat [n_img, img_pitch, D] (rows img_off..img_off+img_tokens of each image are spliced); vid_feat [n_vid, n_tok, D]."""
    _chk(ids, "input_ids", torch.int64); _chk(table, "embed_tokens")
    B, S = ids.shape
    D = table.shape[1]
    out = torch.empty(B, S, D, device=ids.device, dtype=table.dtype)
    if img_feat is not None:
        _chk(img_feat, "img_feat", table.dtype)
        img_pitch = img_pitch or img_feat.shape[-2]
        img_tokens = img_tokens or img_pitch - img_off
    n_vid = 0
    if vid_feat is not None:
        _chk(vid_feat, "vid_feat", table.dtype)
        n_vid = vid_feat.shape[-2]
    sfx, De = _copy_sfx(table.dtype, D)
    _lib.call("ull_embed_splice_" + sfx, _p(ids), _p(table), _p(img_feat), img_tokens, img_pitch, img_off, _p(vid_feat), n_vid, _p(spans),
              _p(out), B, S, De, table.shape[0], _stream())
    return out


def greedy_step(logits_last: torch.Tensor, unfinished: torch.Tensor, eos_ids: Optional[torch.Tensor], pad: Optional[int], seq: torch.Tensor,
                pos: int, alive: torch.Tensor) -> None:
    """One greedy step's bookkeeping in one launch (see ull_greedy_step_*): logits_last [B, V] (rows may be strided), unfinished int32 [B]
    (updated), eos_ids int64 [n] or None, seq int64 [B, L] (column `pos` written), alive int32 [1] (+= rows still unfinished)."""
    _chk(logits_last, "logits"); _chk(unfinished, "unfinished", torch.int32); _chk(seq, "seq", torch.int64); _chk(alive, "alive", torch.int32)
    B, V = logits_last.shape
    if seq.stride(1) != 1 or not unfinished.is_contiguous():
        raise RuntimeError("u-llava_amd.greedy_step: seq rows / unfinished must be contiguous")
    n_eos = 0
    if eos_ids is not None:
        _chk(eos_ids, "eos_ids", torch.int64)
        n_eos = eos_ids.numel()
    _lib.call("ull_greedy_step_" + _SFX[logits_last.dtype], _p(logits_last), logits_last.stride(0), B, V, _p(unfinished), _p(eos_ids), n_eos,
              int(pad) if pad is not None else 0, int(pad is not None), _p(seq), seq.stride(0), int(pos), _p(alive), _stream())


SAMPLE_MAX_V = _D["ULL_SAMPLE_MAX_V"]        # the longest row sample_step stages in LDS


def sample_step(logits_last: torch.Tensor, noise: torch.Tensor, temperature: float, top_k: Optional[int], top_p: Optional[float],
                unfinished: torch.Tensor, eos_ids: Optional[torch.Tensor], pad: Optional[int], seq: torch.Tensor, pos: int,
                alive: torch.Tensor) -> None:
    """One sampled step in one launch (see ull_sample_step): the token of every row is drawn from HF's distribution (`sampling_probs`:
    temperature, top_k, top_p) with the caller's noise, fp32 [B, V] filled by `torch.empty(B, V).exponential_()` -- what
    torch.multinomial(probs, 1) draws and divides by -- and the bookkeeping is greedy_step's.  top_k None / 0 and top_p None / >= 1 are off."""
    _chk(logits_last, "logits"); _chk(unfinished, "unfinished", torch.int32); _chk(seq, "seq", torch.int64); _chk(alive, "alive", torch.int32)
    _chk(noise, "noise", torch.float32)
    B, V = logits_last.shape
    if seq.stride(1) != 1 or not unfinished.is_contiguous() or logits_last.stride(1) != 1:
        raise RuntimeError("u-llava_amd.sample_step: logits rows / seq rows / unfinished must be contiguous")
    if tuple(noise.shape) != (B, V) or not noise.is_contiguous():
        raise RuntimeError(f"u-llava_amd.sample_step: noise must be a contiguous fp32 [{B}, {V}] tensor, got {tuple(noise.shape)}")
    if not temperature > 0:
        raise ValueError(f"u-llava_amd.sample_step: temperature must be positive, got {temperature}")
    n_eos = 0
    if eos_ids is not None:
        _chk(eos_ids, "eos_ids", torch.int64)
        n_eos = eos_ids.numel()
    _lib.call("ull_sample_step", _p(logits_last), DT_CODE[logits_last.dtype], logits_last.stride(0), B, V, _p(noise), float(temperature),
              int(top_k) if top_k is not None and top_k > 0 else 0, float(top_p) if top_p is not None and top_p < 1.0 else 1.0, _p(unfinished),
              _p(eos_ids), n_eos, int(pad) if pad is not None else 0, int(pad is not None), _p(seq), seq.stride(0), int(pos), _p(alive), _stream())


SPEC_MAX_DRAFT = _D["ULL_SPEC_MAX_DRAFT"]         # most draft tokens of one spec_step (16 rows: the few-query limit of the fp8-cache attention)


def spec_step(logits: torch.Tensor, noise: Optional[torch.Tensor], temperature: float, top_k: Optional[int], top_p: Optional[float],
              buf: torch.Tensor, n: int, d: int, n_max: int, eos_ids: Optional[torch.Tensor], num_tokens: int, max_ngram: int,
              picks: torch.Tensor, record: torch.Tensor) -> None:
    """One step of prompt-lookup speculative decoding at batch 1 in two launches (see ull_spec_step): logits [1 + d, V] of the forward over
    buf[0, n-1 : n+d] (buf int64 [1, L]: n valid ids, then the d drafts); noise None picks every row's token as greedy_step does, else as
    sample_step does from noise fp32 [1 + d, V].  The accepted drafts' tokens and the bonus token are written to buf[0, n:], cut at n_max
    valid ids and after the first EOS id; the next step's drafts (`generation.prompt_lookup_candidates` over the new valid ids, at most
    num_tokens) follow them; record int32 [3] = (emitted, finished, next d).  picks: int32 [16] scratch."""
    _chk(logits, "logits"); _chk(buf, "buf", torch.int64); _chk(picks, "picks", torch.int32); _chk(record, "record", torch.int32)
    R, V = logits.shape
    if R != 1 + d or logits.stride(1) != 1:
        raise RuntimeError(f"u-llava_amd.spec_step: logits must be [1 + d = {1 + d}, V] with contiguous rows, got {tuple(logits.shape)}")
    if buf.dim() != 2 or buf.shape[0] != 1 or buf.stride(1) != 1 or picks.numel() < 16 or record.numel() < 3 or not picks.is_contiguous() \
            or not record.is_contiguous():
        raise RuntimeError("u-llava_amd.spec_step: buf must be one contiguous row [1, L], picks int32 [16], record int32 [3]")
    if noise is not None:
        _chk(noise, "noise", torch.float32)
        if tuple(noise.shape) != (R, V) or not noise.is_contiguous():
            raise RuntimeError(f"u-llava_amd.spec_step: noise must be a contiguous fp32 [{R}, {V}] tensor, got {tuple(noise.shape)}")
        if not temperature > 0:
            raise ValueError(f"u-llava_amd.spec_step: temperature must be positive, got {temperature}")
    n_eos = 0
    if eos_ids is not None:
        _chk(eos_ids, "eos_ids", torch.int64)
        n_eos = eos_ids.numel()
    _lib.call("ull_spec_step", _p(logits), DT_CODE[logits.dtype], logits.stride(0), V, _p(noise), float(temperature) if noise is not None else 1.0,
              int(top_k) if top_k is not None and top_k > 0 else 0, float(top_p) if top_p is not None and top_p < 1.0 else 1.0, _p(buf),
              buf.shape[1], int(n), int(d), int(n_max), _p(eos_ids), n_eos, int(num_tokens), int(max_ngram), _p(picks), _p(record), _stream())


def token_logprobs(logits: torch.Tensor, ids: torch.Tensor, row_mask: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """log_softmax(logits.float(), -1)[r, ids[r]] of every row in one launch (see ull_token_logprobs), fp32 [R].  logits [R, V] bf16 / fp16 /
    fp32, rows may be strided (`out.logits[:, -1]`); ids int64 [R] with any element stride (a column `buf[:, pos]` of the generate buffer);
    row_mask int32 [R] contiguous or None.  A row whose id is outside [0, V) (-100 included) or whose row_mask is 0 gets exactly 0.0.
    out: fp32 [R] with any element stride (a column of a [B, n] buffer), returned."""
    _chk(logits, "logits")
    if logits.dim() != 2:
        raise RuntimeError(f"u-llava_amd.token_logprobs: logits must be [R, V], got {tuple(logits.shape)}")
    R, V = logits.shape
    if not ids.is_cuda:
        raise RuntimeError("u-llava_amd: `ids` must live on the GPU (no CPU path exists)")
    if ids.dtype != torch.int64 or tuple(ids.shape) != (R,):
        raise RuntimeError(f"u-llava_amd.token_logprobs: ids must be torch.int64 [{R}], got {ids.dtype} {tuple(ids.shape)}")
    if row_mask is not None:
        _chk(row_mask, "row_mask", torch.int32)
        if tuple(row_mask.shape) != (R,):
            raise RuntimeError(f"u-llava_amd.token_logprobs: row_mask must be int32 [{R}], got {tuple(row_mask.shape)}")
    if out is None:
        out = torch.empty(R, device=logits.device, dtype=F32)
    elif not out.is_cuda or out.dtype != F32 or tuple(out.shape) != (R,):
        raise RuntimeError(f"u-llava_amd.token_logprobs: out must be a GPU torch.float32 [{R}] tensor, got {out.dtype} {tuple(out.shape)}")
    if V == 0 or any(t.dim() and t.stride(0) < 0 for t in (logits, ids, out)):
        raise RuntimeError("u-llava_amd.token_logprobs: empty rows / negative strides are not supported")
    if R:
        _lib.call("ull_token_logprobs", _p(logits), DT_CODE[logits.dtype], logits.stride(0), R, V, _p(ids), ids.stride(0), _p(row_mask), _p(out),
                  out.stride(0) if R > 1 else 1, _stream())
    return out


def ngram_ban(logits: torch.Tensor, ids: torch.Tensor, cur_len: int, ngram: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """HF's NoRepeatNGramLogitsProcessor in one launch (see ull_ngram_ban): out = logits bit for bit, with -inf at the tokens
    `generation.no_repeat_ngram_banned_tokens(ids[:, :cur_len], ngram)` names (those outside [0, V) skipped).  logits [R, V] bf16 / fp16 /
    fp32, rows may be strided (`out.logits[:, -1]`); ids int64 [R, >= cur_len] with contiguous rows of any pitch (the generate buffer);
    out: [R, V] of the logits' dtype with contiguous rows, not overlapping logits; allocated when None, returned."""
    _chk(logits, "logits")
    if logits.dim() != 2:
        raise RuntimeError(f"u-llava_amd.ngram_ban: logits must be [R, V], got {tuple(logits.shape)}")
    R, V = logits.shape
    _chk(ids, "ids", torch.int64)
    cur_len, ngram = int(cur_len), int(ngram)
    if ngram < 1 or cur_len < 0:
        raise ValueError(f"u-llava_amd.ngram_ban: ngram must be >= 1 and cur_len >= 0, got ngram = {ngram}, cur_len = {cur_len}")
    if ids.dim() != 2 or ids.shape[0] != R or ids.shape[1] < cur_len:
        raise RuntimeError(f"u-llava_amd.ngram_ban: ids must be torch.int64 [{R}, >= {cur_len}], got {tuple(ids.shape)}")
    if out is None:
        out = torch.empty(R, V, device=logits.device, dtype=logits.dtype)
    else:
        _chk(out, "out", logits.dtype)
        if tuple(out.shape) != (R, V):
            raise RuntimeError(f"u-llava_amd.ngram_ban: out must be [{R}, {V}], got {tuple(out.shape)}")
    if V == 0 or any(t.stride(0) < 0 for t in (logits, ids, out)) or (R > 1 and out.stride(0) < V):
        raise RuntimeError("u-llava_amd.ngram_ban: empty rows / negative strides / overlapping rows of `out` are not supported")
    if R:
        esz = logits.element_size()
        lo, oo = logits.data_ptr(), out.data_ptr()
        if lo < oo + ((R - 1) * out.stride(0) + V) * esz and oo < lo + ((R - 1) * logits.stride(0) + V) * esz:
            raise RuntimeError("u-llava_amd.ngram_ban: `out` must not overlap `logits` (the ban is not applied in place)")
        _lib.call("ull_ngram_ban", _p(logits), DT_CODE[logits.dtype], logits.stride(0), R, V, _p(ids), ids.stride(0), cur_len, ngram, _p(out),
                  max(out.stride(0), V), _stream())
    return out


# the limits of stop_strings: how many strings, the bytes of one, the bytes of the table's longest token, the LDS window per row
STOP_MAX_STRINGS, STOP_MAX_BYTES, STOP_MAX_TOKEN_BYTES, STOP_MAX_WINDOW = (_D["ULL_STOP_MAX_" + n] for n in ("STRINGS", "BYTES", "TOKEN_BYTES", "WINDOW"))


class StopTable:
    """`generation.token_byte_table`'s (offsets int32 [V + 1], bytes uint8 [n]) checked on the host and copied to `device`: what
    stop_strings reads a token's bytes from.  A table whose longest token is above STOP_MAX_TOKEN_BYTES is refused (ValueError)."""

    def __init__(self, offsets: torch.Tensor, data: torch.Tensor, device):
        offsets, data = torch.as_tensor(offsets), torch.as_tensor(data)
        if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2 or data.dtype != torch.uint8 or data.dim() != 1:
            raise RuntimeError("u-llava_amd.StopTable: offsets must be torch.int32 [V + 1] and bytes torch.uint8 [n]")
        host = offsets.cpu()
        lens = host[1:] - host[:-1]
        if int(host[0]) != 0 or int(host[-1]) != data.numel() or bool((lens < 0).any()):
            raise RuntimeError("u-llava_amd.StopTable: offsets must ascend from 0 to the number of bytes")
        self.V, self.n_bytes, self.max_token_bytes = host.numel() - 1, data.numel(), int(lens.max())
        if self.max_token_bytes > STOP_MAX_TOKEN_BYTES:
            raise ValueError(f"u-llava_amd.StopTable: the longest token has {self.max_token_bytes} bytes, above the limit of {STOP_MAX_TOKEN_BYTES} "
                             "(ULL_STOP_MAX_TOKEN_BYTES)")
        self.offsets, self.bytes = offsets.to(device).contiguous(), data.to(device).contiguous()


class StopStrings:
    """The stop strings of one generate() call as stop_strings takes them: `stops` is a list of non-empty byte strings (the UTF-8 of the
    strings).  The offsets stay on the host (the entry reads and checks them before it launches), the bytes go to `device`.  More than
    STOP_MAX_STRINGS strings, or one longer than STOP_MAX_BYTES bytes: ValueError."""

    def __init__(self, stops, device):
        stops = [bytes(s) for s in stops]
        if not stops or any(len(s) == 0 for s in stops):
            raise ValueError("u-llava_amd.StopStrings: at least one stop string, none of them empty")
        if len(stops) > STOP_MAX_STRINGS:
            raise ValueError(f"u-llava_amd.StopStrings: {len(stops)} stop strings, above the limit of {STOP_MAX_STRINGS} (ULL_STOP_MAX_STRINGS)")
        if max(len(s) for s in stops) > STOP_MAX_BYTES:
            raise ValueError(f"u-llava_amd.StopStrings: a stop string of {max(len(s) for s in stops)} bytes, above the limit of {STOP_MAX_BYTES} "
                             "(ULL_STOP_MAX_BYTES)")
        self.stops = stops
        off = [0]
        for s in stops:
            off.append(off[-1] + len(s))
        self.offsets = torch.tensor(off, dtype=torch.int32)                                   # host memory, kept alive by this object
        self.bytes = torch.frombuffer(bytearray(b"".join(stops)), dtype=torch.uint8).to(device)


def stop_strings(ids: torch.Tensor, L0: int, cur_len: int, table: StopTable, stops: StopStrings, live: torch.Tensor, alive: torch.Tensor) -> None:
    """generate(stop_strings=)'s step in one launch (see ull_stop_strings; `generation.stop_strings_reference` is the rule): every row r
    with live[r] != 0 in whose text -- the table bytes of ids[r, L0:cur_len] -- a stop string ends inside the bytes of the last token
    ids[r, cur_len-1] gets live[r] = 0 and is taken out of alive[0].  ids int64 [R, >= cur_len] with contiguous rows of any pitch (the
    generate buffer); live int32 [R] contiguous (greedy_step's `unfinished`); alive int32 [1] (the step's counter)."""
    _chk(ids, "ids", torch.int64); _chk(live, "live", torch.int32); _chk(alive, "alive", torch.int32)
    if not isinstance(table, StopTable) or not isinstance(stops, StopStrings):
        raise RuntimeError("u-llava_amd.stop_strings: table must be an ops.StopTable and stops an ops.StopStrings")
    _chk(table.offsets, "table.offsets", torch.int32); _chk(table.bytes, "table.bytes", torch.uint8); _chk(stops.bytes, "stops.bytes", torch.uint8)
    L0, cur_len = int(L0), int(cur_len)
    if ids.dim() != 2 or L0 < 0 or cur_len <= L0 or ids.shape[1] < cur_len:
        raise RuntimeError(f"u-llava_amd.stop_strings: ids must be torch.int64 [R, >= cur_len] with 0 <= L0 < cur_len, got {tuple(ids.shape)}, "
                           f"L0 = {L0}, cur_len = {cur_len}")
    R = ids.shape[0]
    if tuple(live.shape) != (R,) or not live.is_contiguous() or alive.numel() != 1:
        raise RuntimeError(f"u-llava_amd.stop_strings: live must be a contiguous int32 [{R}] and alive int32 [1], got {tuple(live.shape)}, {tuple(alive.shape)}")
    if R > 1 and ids.stride(0) < 0:
        raise RuntimeError("u-llava_amd.stop_strings: negative strides are not supported")
    if R:
        _lib.call("ull_stop_strings", _p(ids), ids.stride(0) if R > 1 else ids.shape[1], R, L0, cur_len, _p(table.offsets), _p(table.bytes), table.V,
                  table.n_bytes, table.max_token_bytes, stops.offsets.data_ptr(), _p(stops.bytes), len(stops.stops), _p(live), _p(alive), _stream())


BEAM_MAX_K, BEAM_MAX_CAND =_D["ULL_BEAM_MAX_K"], _D["ULL_BEAM_MAX_CAND"]
BEAM_EARLY_STOPPING = {False: 0, True: 1, "never": 2}


def beam_candidates(num_beams: int, n_eos: int) -> int:
    """KK: how many candidates a beam step keeps per item (HF: max(2, 1 + n_eos) * num_beams)."""
    return max(2, 1 + n_eos) * num_beams


def beam_step(logits: torch.Tensor, pick: Optional[torch.Tensor], run_in: torch.Tensor, run_out: torch.Tensor, pool_in: torch.Tensor,
              pool_out: torch.Tensor, run_sc: torch.Tensor, pool_sc: torch.Tensor, pool_len: torch.Tensor, fin: torch.Tensor, open_: torch.Tensor,
              eos_ids: Optional[torch.Tensor], pad: int, L0: int, cur: int, pow_fin: float, pow_hyp: float, early_stopping, cand_v: torch.Tensor,
              cand_t: torch.Tensor, parent: torch.Tensor, go: torch.Tensor) -> None:
    """One step of beam search for the whole batch in two launches (see ull_beam_step; the rule is generation.beam_search_reference).
    logits [B, Kin, V] bf16 / fp16 / fp32 with Kin in (1, K), rows of one pitch; pick: the same rows after ops.ngram_ban, or None.
    run_in / run_out / pool_in / pool_out int64 [B, K, Lmax] contiguous (in != out), run_sc / pool_sc fp32 [B, K], pool_len / fin int32
    [B, K], open_ int32 [B]: the state, updated; parent int32 [B * K] and go int32 [1]: written; cand_v fp32 / cand_t int32
    [B * K * BEAM_MAX_CAND]: scratch.  pow_fin / pow_hyp: the two powers of the length penalty, rounded to fp32 here."""
    _chk(logits, "logits")
    if logits.dim() != 3:
        raise RuntimeError(f"u-llava_amd.beam_step: logits must be [B, Kin, V], got {tuple(logits.shape)}")
    B, Kin, V = logits.shape
    if run_in.dim() != 3 or run_in.shape[0] != B:
        raise RuntimeError(f"u-llava_amd.beam_step: run_in must be int64 [{B}, K, Lmax], got {tuple(run_in.shape)}")
    K, Lmax = run_in.shape[1:]
    rows, ld = _rows(logits[:, 0] if Kin == 1 else logits)          # (Kin == 1: the rows are the items', whatever the middle stride says)
    pick_ld = 0
    if pick is not None:
        _chk(pick, "pick", logits.dtype)
        if pick.numel() != rows * V or pick.shape[-1] != V:
            raise RuntimeError(f"u-llava_amd.beam_step: pick must hold the logits' {rows} rows of {V}, got {tuple(pick.shape)}")
        pick_ld = _rows(pick.reshape(rows, V) if pick.is_contiguous() else pick[:, 0] if Kin == 1 and pick.dim() == 3 else pick)[1]
    for t, name in ((run_in, "run_in"), (run_out, "run_out"), (pool_in, "pool_in"), (pool_out, "pool_out")):
        _chk(t, name, torch.int64)
        if tuple(t.shape) != (B, K, Lmax) or not t.is_contiguous():
            raise RuntimeError(f"u-llava_amd.beam_step: {name} must be a contiguous int64 [{B}, {K}, {Lmax}], got {tuple(t.shape)}")
    for t, name, dt, n in ((run_sc, "run_sc", F32, B * K), (pool_sc, "pool_sc", F32, B * K), (pool_len, "pool_len", torch.int32, B * K),
                           (fin, "fin", torch.int32, B * K), (open_, "open", torch.int32, B), (parent, "parent", torch.int32, B * K),
                           (go, "go", torch.int32, 1), (cand_v, "cand_v", F32, B * K * BEAM_MAX_CAND), (cand_t, "cand_t", torch.int32, B * K * BEAM_MAX_CAND)):
        _chk(t, name, dt)
        if t.numel() != n or not t.is_contiguous():
            raise RuntimeError(f"u-llava_amd.beam_step: {name} must be a contiguous {dt} tensor of {n} entries, got {tuple(t.shape)}")
    if run_in.data_ptr() == run_out.data_ptr() or pool_in.data_ptr() == pool_out.data_ptr():
        raise RuntimeError("u-llava_amd.beam_step: the ids are double-buffered: run_in / run_out and pool_in / pool_out must differ")
    if Kin not in (1, K) or not 1 <= K <= BEAM_MAX_K or not L0 <= cur < Lmax:
        raise ValueError(f"u-llava_amd.beam_step: Kin must be 1 or K = {K} <= {BEAM_MAX_K} and L0 <= cur < Lmax, got Kin = {Kin}, L0 = {L0}, cur = {cur}, "
                         f"Lmax = {Lmax}")
    n_eos = 0
    if eos_ids is not None:
        _chk(eos_ids, "eos_ids", torch.int64)
        n_eos = eos_ids.numel()
    _lib.call("ull_beam_step", _p(logits), DT_CODE[logits.dtype], ld, _p(pick), pick_ld, B, Kin, K, V, _p(run_in), _p(run_out), _p(pool_in),
              _p(pool_out), _p(run_sc), _p(pool_sc), _p(pool_len), _p(fin), _p(open_), _p(eos_ids), n_eos, int(pad), Lmax, int(L0), int(cur),
              float(pow_fin), float(pow_hyp), BEAM_EARLY_STOPPING[early_stopping], _p(cand_v), _p(cand_t), _p(parent), _p(go), _stream())


def kv_gather_rows(src_k, src_vt, dst_k, dst_vt, n_layers: int, src_rows: int, dst_rows: int, H: int, hd: int, elem_size: int, src_smax: int,
                   dst_smax: int, src_p0: int, dst_p0: int, n: int, row_map: Optional[torch.Tensor], skip: Optional[torch.Tensor]) -> None:
    """Rows of a KV cache copied into another set of buffers in one launch (see ull_kv_gather_rows): positions [dst_p0, dst_p0 + n) of row r
    <- positions [src_p0, src_p0 + n) of source row row_map[r], for every layer, K and V^T, except rows with skip[r] == r.  src_* / dst_*:
    ctypes void* arrays of the per-layer buffers (KVCache.c_ptrs); row_map / skip: int32 [dst_rows] on the device, or None."""
    for t, name in ((row_map, "row_map"), (skip, "skip")):
        if t is not None:
            _chk(t, name, torch.int32)
            if tuple(t.shape) != (dst_rows,) or not t.is_contiguous():
                raise RuntimeError(f"u-llava_amd.kv_gather_rows: {name} must be a contiguous int32 [{dst_rows}], got {tuple(t.shape)}")
    _lib.call("ull_kv_gather_rows", src_k, src_vt, dst_k, dst_vt, n_layers, src_rows, dst_rows, H, hd, elem_size, src_smax, dst_smax, int(src_p0),
              int(dst_p0), int(n), _p(row_map), _p(skip), _stream())


def ids_common_prefix(ids_a: torch.Tensor, ids_b: torch.Tensor, n: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [R]: per row, the length of the common prefix of ids_a[r, :n] and ids_b[r, :n] (see ull_ids_common_prefix), in one launch.
    ids_a / ids_b: int64 [R, >= n] with contiguous rows of any pitch (a slice of the columns of the generate buffer will do)."""
    _chk(ids_a, "ids_a", torch.int64); _chk(ids_b, "ids_b", torch.int64)
    n = int(n)
    if ids_a.dim() != 2 or ids_b.dim() != 2 or ids_a.shape[0] != ids_b.shape[0] or n < 0 or ids_a.shape[1] < n or ids_b.shape[1] < n:
        raise RuntimeError(f"u-llava_amd.ids_common_prefix: need two int64 [R, >= {n}] tensors, got {tuple(ids_a.shape)} and {tuple(ids_b.shape)}")
    R = ids_a.shape[0]
    for t in (ids_a, ids_b):
        if n > 1 and t.stride(1) != 1 or (R > 1 and n > 0 and t.stride(0) < n):
            raise RuntimeError("u-llava_amd.ids_common_prefix: the rows must be contiguous and must not overlap")
    if out is None:
        out = torch.empty(R, dtype=torch.int32, device=ids_a.device)
    else:
        _chk(out, "out", torch.int32)
        if tuple(out.shape) != (R,) or not out.is_contiguous():
            raise RuntimeError(f"u-llava_amd.ids_common_prefix: out must be a contiguous int32 [{R}], got {tuple(out.shape)}")
    _lib.call("ull_ids_common_prefix", _p(ids_a), ids_a.stride(0), _p(ids_b), ids_b.stride(0), R, n, _p(out), _stream())
    return out


def kv8_copy_positions(src, dst, n: int) -> None:
    """Positions [0, n) of every layer of an fp8 KV cache into another set of buffers, in one launch per 32 layers (see
    ull_kv8_copy_positions).  src / dst: (k8 list, vt8 list, k_scale list, vt_scale list) of per-layer tensors -- codes uint8
    [B, H, smax, hd] / [B, H, hd, smax], scales fp32 [B, H, smax]; the two pitches may differ.  Nothing at or beyond position n is written."""
    n = int(n)
    n_layers = len(src[0])
    if len(src) != 4 or len(dst) != 4 or any(len(l) != n_layers for l in tuple(src) + tuple(dst)):
        raise RuntimeError("u-llava_amd.kv8_copy_positions: src and dst are four lists of one tensor per layer each")
    if n_layers == 0:
        return
    B, H, s_smax, hd = src[0][0].shape
    d_smax = dst[0][0].shape[2]
    for lists, smax, side in ((src, s_smax, "src"), (dst, d_smax, "dst")):
        shapes = ((B, H, smax, hd), (B, H, hd, smax), (B, H, smax), (B, H, smax))
        for l, shp, dt in zip(lists, shapes, (torch.uint8, torch.uint8, F32, F32)):
            for t in l:
                _chk(t, side, dt)
                if tuple(t.shape) != shp or not t.is_contiguous():
                    raise RuntimeError(f"u-llava_amd.kv8_copy_positions: a {side} buffer is {tuple(t.shape)}, not a contiguous {shp}")
    if not 0 <= n <= min(s_smax, d_smax):
        raise ValueError(f"u-llava_amd.kv8_copy_positions: {n} positions do not fit caches of {s_smax} and {d_smax}")
    _lib.call("ull_kv8_copy_positions", *[_ptr_array(l) for l in src], *[_ptr_array(l) for l in dst], n_layers, B, H, hd, s_smax, d_smax, n, _stream())


def video_pool(f: torch.Tensor, B: int, T: int, N: int, tok_pitch: Optional[int] = None, tok_off: int = 0) -> torch.Tensor:
    """f [B*T, tok_pitch, D]; patches are tokens tok_off..tok_off+N of every frame."""
    _chk(f, "f")
    D = f.shape[-1]
    out = torch.empty(B, T + N, D, device=f.device, dtype=f.dtype)
    _lib.call("ull_video_pool_" + _SFX[f.dtype], _p(f), _p(out), B, T, N, D, tok_pitch or N, tok_off, _stream())
    return out


def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    _chk(src, "src"); _chk(idx, "idx", torch.int64)
    n, D = idx.numel(), src.shape[-1]
    out = torch.empty(n, D, device=src.device, dtype=src.dtype)
    if n:
        sfx, De = _copy_sfx(src.dtype, D)
        k = De // D
        _lib.call("ull_gather_rows_" + sfx, _p(src), src.stride(-2) * k, _p(idx), _p(out), De, n, De, _stream())
    return out


def add_rows(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """bf16(a + b) with b broadcast over leading rows (b has b_rows rows, a has k*b_rows)."""
    _chk(a, "a"); _chk(b, "b", a.dtype)
    D = a.shape[-1]
    rows, b_rows = a.numel() // D, b.numel() // D
    out = torch.empty_like(a)
    _lib.call("ull_add_rows_" + _SFX[a.dtype], _p(a), _p(b), _p(out), rows, D, b_rows, _stream())
    return out


# ---- SAM --------------------------------------------------------------------------------------------------------------
def window_partition(x: torch.Tensor, B: int, H: int, W: int, ws: int) -> torch.Tensor:
    """x [B*H*W, C] token-major -> [B*nW*ws*ws, C]."""
    _chk(x, "x")
    C = x.shape[-1]
    nW = ((H + ws - 1) // ws) * ((W + ws - 1) // ws)
    out = torch.empty(B * nW * ws * ws, C, device=x.device, dtype=x.dtype)
    sfx, Ce = _copy_sfx(x.dtype, C)
    _lib.call("ull_window_partition_" + sfx, _p(x), _p(out), B, H, W, Ce, ws, _stream())
    return out


def window_unpartition_add(win: torch.Tensor, shortcut: torch.Tensor, B: int, H: int, W: int, ws: int) -> torch.Tensor:
    _chk(win, "win"); _chk(shortcut, "shortcut", win.dtype)
    out = torch.empty_like(shortcut)
    _lib.call("ull_window_unpartition_add_" + _SFX[win.dtype], _p(win), _p(shortcut), _p(out), B, H, W, shortcut.shape[-1], ws, _stream())
    return out


def sam_relpos(q: torch.Tensor, q_strides, rel_pos_h: torch.Tensor, rel_pos_w: torch.Tensor, NB: int, nH: int, KH: int, KW: int, hd: int):
    _chk(q, "q"); _chk(rel_pos_h, "rel_pos_h", q.dtype); _chk(rel_pos_w, "rel_pos_w", q.dtype)
    rel_pos_h, rel_pos_w = fit_rel_pos(rel_pos_h, KH), fit_rel_pos(rel_pos_w, KW)
    oh = torch.empty(NB * nH, KH * KW, KH, device=q.device, dtype=q.dtype)
    ow = torch.empty(NB * nH, KH * KW, KW, device=q.device, dtype=q.dtype)
    _lib.call("ull_sam_relpos_" + _SFX[q.dtype], _p(q), *q_strides, _p(rel_pos_h), _p(rel_pos_w), _p(oh), _p(ow), NB, nH, KH, KW, hd, _stream())
    return oh, ow


def layernorm2d_cl(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-6, gelu: bool = False) -> torch.Tensor:
    _chk(x, "x"); _chk(w, "w", x.dtype); _chk(b, "b", x.dtype)
    if not x.is_contiguous():
        raise RuntimeError("u-llava_amd.layernorm2d_cl: x must be contiguous channels-last rows")
    C = x.shape[-1]
    out = torch.empty_like(x)
    _lib.call("ull_layernorm2d_cl_" + _SFX[x.dtype], _p(x), _p(w), _p(b), _p(out), x.numel() // C, C, float(eps), int(gelu), _stream())
    return out


def neck_layernorm2d_f32(xa: torch.Tensor, xb: Optional[torch.Tensor], xb_scale: float, w: torch.Tensor, b: torch.Tensor, eps: float,
                         split: bool) -> torch.Tensor:
    """LayerNorm2d of the fp16 model's fp32 neck (image_encoder.py:117-124): fp32 rows xa (+ xb * xb_scale) -> fp16.
    split=False: [rows, C] = fp16(y).  split=True: [2, rows, C] = (fp16(y), fp16((y - fp16(y)) * 2^11)), the two-term image of y."""
    _chk(xa, "xa", torch.float32); _chk(w, "w", torch.float16); _chk(b, "b", torch.float16)
    C = xa.shape[-1]
    rows = xa.numel() // C
    if not xa.is_contiguous() or (xb is not None and (not xb.is_contiguous() or xb.shape != xa.shape or xb.dtype != torch.float32)):
        raise RuntimeError("u-llava_amd.neck_layernorm2d_f32: xa / xb must be contiguous fp32 rows of the same shape")
    out = torch.empty((2, rows, C) if split else (rows, C), device=xa.device, dtype=torch.float16)
    _lib.call("ull_neck_layernorm2d_f32in_f16", _p(xa), _p(xb), float(xb_scale), _p(w), _p(b), _p(out), _p(out[1]) if split else None, rows, C,
              float(eps), _stream())
    return out


def im2col3x3(x: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    _chk(x, "x")
    C = x.shape[-1]
    out = torch.empty(B * H * W, 9 * C, device=x.device, dtype=x.dtype)
    _lib.call("ull_im2col3x3_" + _SFX[x.dtype], _p(x), _p(out), B, H, W, C, _stream())
    return out


def mask_matmul(hyper: torch.Tensor, up: torch.Tensor, n: int, T: int, C: int, G: int) -> torch.Tensor:
    _chk(hyper, "hyper"); _chk(up, "up", hyper.dtype)
    out = torch.empty(n, T, 4 * G, 4 * G, device=up.device, dtype=hyper.dtype)
    _lib.call("ull_mask_matmul_" + _SFX[hyper.dtype], _p(hyper), _p(up), _p(out), n, T, C, G, _stream())
    return out


def bilinear(x: torch.Tensor, in_h: int, in_w: int, out_h: int, out_w: int) -> torch.Tensor:
    """x [n, Hfull, Wfull] (bf16 or fp32, contiguous); the top-left in_h x in_w crop of every image is resized -> fp32 [n, out_h, out_w]."""
    if not x.is_cuda or x.dtype not in DT_CODE or not x.is_contiguous():
        raise RuntimeError("u-llava_amd.bilinear: contiguous bf16/fp16/fp32 GPU tensor required")
    n, Hf, Wf = x.shape
    out = torch.empty(n, out_h, out_w, device=x.device, dtype=torch.float32)
    _lib.call("ull_bilinear_f32", _p(x), DT_CODE[x.dtype], Hf * Wf, Wf, in_h, in_w, _p(out), n, out_h, out_w, _stream())
    return out


def _ce_rows(logits: torch.Tensor, labels: torch.Tensor):
    """The one layout rule of the three shifted-CE wrappers -> (B, S, V, ld).  The kernels index row (b, t) as (b * S + t) * ld, so the
    [B, S, V] logits must fold onto rows of ONE pitch (_rows: contiguous, or a [..., :V] view of wider rows); anything else is refused."""
    _chk(logits, "logits"); _chk(labels, "labels", torch.int64)
    if logits.dim() != 3 or tuple(labels.shape) != tuple(logits.shape[:2]):
        raise RuntimeError("u-llava_amd.shifted_cross_entropy: logits [B, S, V] and labels [B, S] required")
    B, S, V = logits.shape
    return B, S, V, _rows(logits)[1]


def shifted_cross_entropy(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """mean CE of logits[:, :-1] against labels[:, 1:] (ignore_index -100) -> 0-dim tensor of the logits' dtype like the reference's loss."""
    acc = shifted_cross_entropy_stats(logits, labels)
    return (acc[0] / acc[1]).to(logits.dtype)


def mask_loss_sums(logits: torch.Tensor, target: torch.Tensor, scale: float = 1000.0) -> torch.Tensor:
    """fp32 [n, 4] = per mask {sum BCE-with-logits, sum (sigmoid/scale)*t, sum sigmoid/scale, sum t/scale} (models/loss.py)."""
    _chk(logits, "mask logits", torch.float32); _chk(target, "mask target", torch.float32)
    if logits.shape != target.shape or not logits.is_contiguous() or not target.is_contiguous():
        raise RuntimeError("u-llava_amd.mask_loss_sums: logits / target must be contiguous and of the same shape")
    n = logits.shape[0]
    part = torch.empty(n, 64, 4, device=logits.device, dtype=torch.float32)
    _lib.call("ull_mask_loss_sums_f32", _p(logits), _p(target), n, logits[0].numel(), float(scale), _p(part), _stream())
    return part.sum(1)


def box_losses(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """fp32 [2] = {sum |pred - gt|, sum (1 - GIoU) over well-formed predictions}; pred [n,4] bf16/fp32, gt [n,4] fp32."""
    if pred.dtype not in DT_CODE:
        raise RuntimeError("u-llava_amd.box_losses: pred must be bf16, fp16 or fp32")
    _chk(pred, "pred boxes", pred.dtype); _chk(gt, "gt boxes", torch.float32)
    out = torch.empty(2, device=pred.device, dtype=torch.float32)
    _lib.call("ull_box_losses_f32", _p(pred.contiguous()), DT_CODE[pred.dtype], _p(gt.contiguous()), pred.shape[0], _p(out), _stream())
    return out


# ---- backward kernels (training path; see autograd_ops.py) ----------------------------------------------------------------------------
def rmsnorm_bwd(x: torch.Tensor, w: torch.Tensor, dy: torch.Tensor, eps: float, need_dw: bool = True):
    """-> (dx like x, dw float32 [D] or None)."""
    _chk(x, "x"); _chk(w, "w", x.dtype); _chk(dy, "dy", x.dtype)
    rows, ldx = _rows(x)
    D = x.shape[-1]
    dx = torch.empty_like(x)
    dw = torch.zeros(D, device=x.device, dtype=torch.float32) if need_dw else None
    _lib.call("ull_rmsnorm_bwd_" + _SFX[x.dtype], _p(x), ldx, _p(w), _p(dy), _rows(dy)[1], _p(dx), _rows(dx)[1], _p(dw), rows, D, float(eps), _stream())
    return dx, dw


def swiglu_fwd(gu: torch.Tensor, halves: bool = False) -> torch.Tensor:
    """gu [M, 2I] -> silu(gate) * up [M, I].  Columns: the 16-wide gate/up interleave of the inference pack, or (halves) [gate | up]."""
    _chk(gu, "gu")
    M, I = gu.numel() // gu.shape[-1], gu.shape[-1] // 2
    a = torch.empty(*gu.shape[:-1], I, device=gu.device, dtype=gu.dtype)
    _lib.call("ull_swiglu_fwd_" + _SFX[gu.dtype], _p(gu.contiguous()), _p(a), M, I, int(halves), _stream())
    return a


def swiglu_bwd(gu: torch.Tensor, da: torch.Tensor, halves: bool = False) -> torch.Tensor:
    _chk(gu, "gu"); _chk(da, "da", gu.dtype)
    M, I = gu.numel() // gu.shape[-1], gu.shape[-1] // 2
    dgu = torch.empty_like(gu)
    _lib.call("ull_swiglu_bwd_" + _SFX[gu.dtype], _p(gu.contiguous()), _p(da.contiguous()), _p(dgu), M, I, int(halves), _stream())
    return dgu


def relu_mask(y: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dx = y > 0 ? dy : 0 (ReLU backward as a selection)."""
    _chk(y, "y"); _chk(dy, "dy", y.dtype)
    y, dy = y.contiguous(), dy.contiguous()
    dx = torch.empty_like(dy)
    _lib.call("ull_relu_mask_" + _SFX[y.dtype], _p(y), _p(dy), _p(dx), y.numel(), _stream())
    return dx


def rope_bwd_inplace(dx: torch.Tensor, row_stride: int, positions: torch.Tensor, inv_freq: torch.Tensor, tokens: int, n_heads: int, hd: int):
    _chk(dx, "dx"); _chk(positions, "positions", torch.int64); _chk(inv_freq, "inv_freq", torch.float32)
    _lib.call("ull_rope_bwd_inplace_" + _SFX[dx.dtype], _p(dx), row_stride, _p(positions), _p(inv_freq), tokens, n_heads, hd, _stream())


def attention_bwd(q, k, v, o, do, dq, dk, dv, strides, key_mask, B: int, H: int, Sq: int, Sk: int, hd: int, causal: bool, mult: float):
    """strides: 8 triples (batch, head, seq) of element strides for q, k, v, o, do, dq, dk, dv (hd contiguous everywhere)."""
    import ctypes
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (o, "o"), (do, "do"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
        _chk(t, n, q.dtype if t is not q else None)
    if key_mask is not None:
        _chk(key_mask, "key_mask", torch.int32)
    flat = [int(x) for tr in strides for x in tr]
    assert len(flat) == 24
    arr = (ctypes.c_int64 * 24)(*flat)
    (q_bs, q_hs, q_ss), (k_bs, k_hs, k_ss), (_, v_hs, _), (_, o_hs, _), (g_bs, g_hs, g_ss) = strides[:5]
    # Three kernel families.  The two matrix-core ones need the heads of Q, K and dO side by side (head stride == hd), every stride 8-byte
    # and every token stride 16-byte aligned, and at hd 128 the head strides of V and O 16-byte aligned too (what ull_attention_bwd_mfma_
    # checks); any other layout or head dim runs the scalar kernels below.
    matrix = (hd in (64, 128) and q_hs == hd and k_hs == hd and g_hs == hd and all(x % 4 == 0 for x in flat)
              and all(flat[i] % 8 == 0 for i in range(2, 24, 3)) and (hd != 128 or (v_hs % 8 == 0 and o_hs % 8 == 0)))
    if matrix:
        # hd 128 (the LLaMA block): attn_bwd_*_tiles_kernel -- operand tiles staged through the LDS, transposed fragments from the
        # transposing LDS read.  hd 64: attn_bwd_*_mfma_kernel<64> -- fragments straight from global memory; Q, K and dO also as
        # transpose_v images.
        pitch = ((max(Sq, Sk) + 63) // 64) * 64
        qt = kt = gt = None
        if hd != 128:
            qt = transpose_v(q, q_bs, q_ss, B, Sq, H, hd, pitch)
            kt = transpose_v(k, k_bs, k_ss, B, Sk, H, hd, pitch)
            gt = transpose_v(do, g_bs, g_ss, B, Sq, H, hd, pitch)
        scratch = torch.empty(2 * B * H * (((Sq + 63) // 64) * 64), device=q.device, dtype=torch.float32)
        _lib.call("ull_attention_bwd_mfma_" + _SFX[q.dtype], _p(q), _p(k), _p(v), _p(o), _p(do), _p(qt), _p(kt), _p(gt), pitch, _p(dq), _p(dk), _p(dv),
                  arr, _p(key_mask), B, H, Sq, Sk, hd, int(causal), float(mult), _p(scratch), _stream())
        return
    # scalar kernels: any head dim <= 128, any strides
    scratch = torch.empty(2 * B * H * Sq, device=q.device, dtype=torch.float32)
    _lib.call("ull_attention_bwd_" + _SFX[q.dtype], _p(q), _p(k), _p(v), _p(o), _p(do), _p(dq), _p(dk), _p(dv), arr, _p(key_mask), B, H, Sq, Sk, hd,
              int(causal), float(mult), _p(scratch), _stream())


def shifted_cross_entropy_stats(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """float32 [2] = {sum of token losses, counted tokens} of the shifted CE (the loss is stats[0] / stats[1])."""
    B, S, V, ld = _ce_rows(logits, labels)
    acc = torch.zeros(2, device=logits.device, dtype=torch.float32)
    _lib.call("ull_shifted_cross_entropy_" + _SFX[logits.dtype], _p(logits), ld, _p(labels.contiguous()), B, S, V, _p(acc), _stream())
    return acc


def shifted_cross_entropy_bwd(logits: torch.Tensor, labels: torch.Tensor, stats: torch.Tensor, gout: torch.Tensor) -> torch.Tensor:
    """dlogits [B, S, V] at the row pitch of `logits` (the kernel takes ONE pitch for both: a [..., :V] view of padded rows gets a gradient
    with the same padded rows, whose pad columns are never written)."""
    _chk(stats, "stats", torch.float32); _chk(gout, "gout", torch.float32)
    B, S, V, ld = _ce_rows(logits, labels)
    dl = torch.empty_strided((B, S, V), (S * ld, ld, 1), device=logits.device, dtype=logits.dtype)
    _lib.call("ull_shifted_cross_entropy_bwd_" + _SFX[logits.dtype], _p(logits), ld, _p(labels.contiguous()), B, S, V, _p(stats),
              _p(gout), _p(dl), _stream())
    return dl


def embed_splice_bwd(ids, demb, vocab: int, img_shape=None, vid_shape=None, spans=None, img_tokens: int = 0, img_pitch: int = 0, img_off: int = 0,
                     need_table: bool = True, vid_tokens: int = 0, detach_text: bool = False):
    """-> (d_table float32 [vocab, D] or None, d_img [n_img, pitch, D] or None, d_vid or None); rows not written stay zero.
    img_tokens / vid_tokens: span lengths (needed even when d_img / d_vid are not: span rows never reach the table).
    detach_text: projector_from_scratch -- only the start / end token rows of samples with an image / video reach the table."""
    _chk(ids, "input_ids", torch.int64); _chk(demb, "demb")
    B, S = ids.shape
    D = demb.shape[-1]
    d_table = torch.zeros(vocab, D, device=demb.device, dtype=torch.float32) if need_table else None
    d_img = torch.zeros(img_shape, device=demb.device, dtype=demb.dtype) if img_shape is not None else None
    d_vid = torch.zeros(vid_shape, device=demb.device, dtype=demb.dtype) if vid_shape is not None else None
    n_vid = vid_shape[-2] if vid_shape is not None else vid_tokens
    _lib.call("ull_embed_splice_bwd_" + _SFX[demb.dtype], _p(ids), _p(demb.contiguous()), _p(d_table), _p(d_img), img_tokens, img_pitch, img_off,
              _p(d_vid), n_vid, _p(spans), B, S, D, vocab, int(detach_text), _stream())
    return d_table, d_img, d_vid


def transpose2d(x: torch.Tensor) -> torch.Tensor:
    """[R, C] (last dim contiguous, any row stride) -> fresh contiguous [C, R]."""
    _chk(x, "x")
    if x.dim() != 2:
        raise RuntimeError("u-llava_amd.transpose2d: needs a 2-D tensor")
    R, C = x.shape
    y = torch.empty(C, R, device=x.device, dtype=x.dtype)
    _lib.call("ull_transpose2d_" + _SFX[x.dtype], _p(x), x.stride(0) if R > 1 else C, _p(y), R, R, C, _stream())
    return y


def colsum(x: torch.Tensor) -> torch.Tensor:
    """float32 [N] column sums of x [rows, N]."""
    _chk(x, "x")
    rows, ld = _rows(x)
    out = torch.empty(x.shape[-1], device=x.device, dtype=torch.float32)
    _lib.call("ull_colsum_" + _SFX[x.dtype], _p(x), ld, rows, x.shape[-1], _p(out), _stream())
    return out


def sum_slabs(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """x [R, n] -> scale * sum over R (fp32 accumulation), same dtype."""
    _chk(x, "x")
    if not x.is_contiguous() or x.dim() != 2:
        raise RuntimeError("u-llava_amd.sum_slabs: contiguous [R, n] required")
    out = torch.empty(x.shape[1], device=x.device, dtype=x.dtype)
    _lib.call("ull_sum_slabs_" + _SFX[x.dtype], _p(x), _p(out), x.shape[0], x.shape[1], float(scale), _stream())
    return out


def layernorm_bwd(x, w, dy, eps: float, need_wb: bool = True):
    """-> (dx, dw float32 [D] or None, db float32 [D] or None)."""
    _chk(x, "x"); _chk(w, "w", x.dtype); _chk(dy, "dy", x.dtype)
    rows, ldx = _rows(x)
    D = x.shape[-1]
    dx = torch.empty_like(x)
    dw = torch.zeros(D, device=x.device, dtype=torch.float32) if need_wb else None
    db = torch.zeros(D, device=x.device, dtype=torch.float32) if need_wb else None
    _lib.call("ull_layernorm_bwd_" + _SFX[x.dtype], _p(x), ldx, _p(w), _p(dy), _rows(dy)[1], _p(dx), _rows(dx)[1], _p(dw), _p(db), rows, D, float(eps),
              _stream())
    return dx, dw, db


def layernorm2d_cl_bwd(x, w, b, dy, eps: float, gelu: bool, need_wb: bool = True):
    _chk(x, "x"); _chk(w, "w", x.dtype); _chk(b, "b", x.dtype); _chk(dy, "dy", x.dtype)
    C = x.shape[-1]
    dx = torch.empty_like(x)
    dw = torch.zeros(C, device=x.device, dtype=torch.float32) if need_wb else None
    db = torch.zeros(C, device=x.device, dtype=torch.float32) if need_wb else None
    _lib.call("ull_layernorm2d_cl_bwd_" + _SFX[x.dtype], _p(x.contiguous()), _p(w), _p(b), _p(dy.contiguous()), _p(dx), _p(dw), _p(db), x.numel() // C, C,
              float(eps), int(gelu), _stream())
    return dx, dw, db


def gelu_fwd(x):
    _chk(x, "x")
    y = torch.empty_like(x)
    _lib.call("ull_gelu_fwd_" + _SFX[x.dtype], _p(x.contiguous()), _p(y), x.numel(), _stream())
    return y


def gelu_bwd(x, dy):
    _chk(x, "x"); _chk(dy, "dy", x.dtype)
    dx = torch.empty_like(x)
    _lib.call("ull_gelu_bwd_" + _SFX[x.dtype], _p(x.contiguous()), _p(dy.contiguous()), _p(dx), x.numel(), _stream())
    return dx


def mask_matmul_bwd(hyper, up, dmasks, n: int, T: int, C: int, G: int):
    """-> (dhyper float32 [n, T, C], dup like up)."""
    _chk(hyper, "hyper"); _chk(up, "up", hyper.dtype); _chk(dmasks, "dmasks", hyper.dtype)
    dh = torch.zeros(n, T, C, device=up.device, dtype=torch.float32)
    dup = torch.empty_like(up)
    _lib.call("ull_mask_matmul_bwd_" + _SFX[hyper.dtype], _p(hyper.contiguous()), _p(up), _p(dmasks.contiguous()), _p(dh), _p(dup), n, T, C, G, _stream())
    return dh, dup


def mask_loss_sums_bwd(logits, target, g, scale: float = 1000.0):
    _chk(logits, "mask logits", torch.float32); _chk(target, "mask target", torch.float32); _chk(g, "g", torch.float32)
    n = logits.shape[0]
    dl = torch.empty_like(logits)
    _lib.call("ull_mask_loss_sums_bwd_f32", _p(logits.contiguous()), _p(target.contiguous()), _p(g.contiguous()), n, logits[0].numel(), float(scale),
              _p(dl), _stream())
    return dl


def box_losses_bwd(pred, gt, gw):
    _chk(pred, "pred boxes", pred.dtype if pred.dtype in DT_CODE else None); _chk(gt, "gt boxes", torch.float32); _chk(gw, "gw", torch.float32)
    dp = torch.empty(pred.shape[0], 4, device=pred.device, dtype=torch.float32)
    _lib.call("ull_box_losses_bwd_f32", _p(pred.contiguous()), DT_CODE[pred.dtype], _p(gt.contiguous()), pred.shape[0], _p(gw.contiguous()), _p(dp),
              _stream())
    return dp


def bilinear_bwd(dout, full_hw, in_h: int, in_w: int):
    """adjoint of bilinear(): dout fp32 [n, out_h, out_w] -> din fp32 [n, Hfull, Wfull] (zero outside the in_h x in_w crop)."""
    _chk(dout, "dout", torch.float32)
    n, oh, ow = dout.shape
    Hf, Wf = full_hw
    din = torch.zeros(n, Hf, Wf, device=dout.device, dtype=torch.float32)
    _lib.call("ull_bilinear_bwd_f32", _p(dout.contiguous()), _p(din), Hf * Wf, Wf, in_h, in_w, n, oh, ow, _stream())
    return din


# ---- fused two-way mask decoder (csrc/sam_decoder.hip) ------------------------------------------------------------------------------
def _lin_ptrs(*lins):
    out = []
    for l in lins:
        out += [_p(l.weight), _p(l.bias)]
    return out


def _proj_args(projs, n: int, T: int, like: torch.Tensor):
    """projs: list of up to 3 (linear holder, add_pe) -> (ctypes pointer array or None, ctypes int array or None, output tensors)."""
    import ctypes
    if not projs:
        return None, None, []
    outs, ptrs, flags = [], [], []
    for lin, add_pe in projs:
        o = torch.empty(n, T, lin.weight.shape[0], device=like.device, dtype=like.dtype)
        outs.append(o)
        ptrs += [_p(lin.weight), _p(lin.bias), _p(o)]
        flags.append(int(add_pe))
    while len(flags) < 3:
        ptrs += [None, None, None]
        flags.append(0)
    return (ctypes.c_void_p * 9)(*ptrs), (ctypes.c_int * 3)(*flags), outs


def sam_self_attn_heads(queries, qpe, a, first: bool):
    """queries / qpe [n, T, 256] -> concatenated head outputs [n, T, 256] of the token self attention (before out_proj)."""
    _chk(queries, "queries"); _chk(qpe, "qpe", queries.dtype)
    n, T, _ = queries.shape
    att = torch.empty_like(queries)
    _lib.call("ull_sam_self_attn_heads_" + _SFX[queries.dtype], _p(queries), _p(qpe), n, T, int(first), *_lin_ptrs(a.q_proj, a.k_proj, a.v_proj), _p(att),
              _stream())
    return att


def sam_out_ln(att, res, qpe, out_proj, ln, projs=None, eps: float = 1e-5):
    """LayerNorm(res + out_proj(att)) (res None: no residual) + token-side projections for the next attention -> (out, [proj outputs])."""
    _chk(att, "att"); _chk(qpe, "qpe", att.dtype)
    n, T, din = att.shape
    out = torch.empty(n, T, 256, device=att.device, dtype=att.dtype)
    pa, fa, outs = _proj_args(projs, n, T, att)
    _lib.call("ull_sam_out_ln_" + _SFX[att.dtype], _p(att), din, _p(res), _p(qpe), n, T, _p(out_proj.weight), _p(out_proj.bias), _p(ln.weight), _p(ln.bias),
              float(eps), _p(out), pa, fa, _stream())
    return out, outs


def sam_token_mlp_ln(queries, qpe, lin1, lin2, ln, projs=None, eps: float = 1e-5):
    _chk(queries, "queries"); _chk(qpe, "qpe", queries.dtype)
    n, T, _ = queries.shape
    hidden = lin1.weight.shape[0]
    ws = torch.empty(n * (hidden // 256) * 8 * 256, device=queries.device, dtype=torch.float32)
    out = torch.empty_like(queries)
    pa, fa, outs = _proj_args(projs, n, T, queries)
    _lib.call("ull_sam_token_mlp_ln_" + _SFX[queries.dtype], _p(queries), _p(qpe), n, T, hidden, *_lin_ptrs(lin1, lin2), _p(ln.weight), _p(ln.bias),
              float(eps), _p(ws), _p(out), pa, fa, _stream())
    return out, outs


def sam_small_mlps(hs, hyper_mlps, iou_head):
    """hs [n, T, 256] -> (hyper [n, 4, C], iou [n, n_iou]): the 4 hyper-network MLPs on rows 1..4 and the IoU head on row 0."""
    import ctypes
    _chk(hs, "hs")
    n, T, _ = hs.shape
    ptrs = []
    for m in list(hyper_mlps) + [iou_head]:
        ptrs += _lin_ptrs(*m.layers)
    arr = (ctypes.c_void_p * 30)(*ptrs)
    C, n_iou = hyper_mlps[0].layers[2].weight.shape[0], iou_head.layers[2].weight.shape[0]
    hyper = torch.empty(n, 4, C, device=hs.device, dtype=hs.dtype)
    iou = torch.empty(n, n_iou, device=hs.device, dtype=hs.dtype)
    _lib.call("ull_sam_small_mlps_" + _SFX[hs.dtype], _p(hs), n, T, arr, 4, C, n_iou, _p(hyper), _p(iou), _stream())
    return hyper, iou


def sam_t2i_attention(qproj, keys, pos, a, late_bias_kv: bool):
    """token -> image attention core: qproj [n, T, 128], keys [n, P, 256], pos [P, 256] -> attention output [n, T, 128] (before out_proj)."""
    _chk(qproj, "qproj"); _chk(keys, "keys", qproj.dtype); _chk(pos, "pos", qproj.dtype)
    n, T, _ = qproj.shape
    P = keys.shape[1]
    ws_s = torch.empty(n * 8 * 8 * P, device=keys.device, dtype=keys.dtype)
    ws_v = torch.empty(n * P * 128, device=keys.device, dtype=keys.dtype)
    att = torch.empty(n, T, 128, device=keys.device, dtype=keys.dtype)
    _lib.call("ull_sam_t2i_attention_" + _SFX[qproj.dtype], _p(qproj), _p(keys), _p(pos), n, T, P, *_lin_ptrs(a.k_proj, a.v_proj), int(late_bias_kv),
              _p(ws_s), _p(ws_v), _p(att), _stream())
    return att


def sam_i2t_attention_ln(keys, pos, kproj, vproj, a, ln, late_bias_q: bool, eps: float = 1e-5):
    """image -> token attention + residual + LayerNorm in one launch -> new keys [n, P, 256]."""
    _chk(keys, "keys"); _chk(pos, "pos", keys.dtype); _chk(kproj, "kproj", keys.dtype); _chk(vproj, "vproj", keys.dtype)
    n, T, _ = kproj.shape
    P = keys.shape[1]
    out = torch.empty_like(keys)
    _lib.call("ull_sam_i2t_attention_ln_" + _SFX[keys.dtype], _p(keys), _p(pos), _p(kproj), _p(vproj), n, T, P, *_lin_ptrs(a.q_proj, a.out_proj),
              int(late_bias_q), _p(ln.weight), _p(ln.bias), float(eps), _p(out), _stream())
    return out


# ---- optimizer kernels (csrc/optim.hip; host: optim.py) --------------------------------------------------------------------------------
def adamw_step(master: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grad: torch.Tensor, param_out: Optional[torch.Tensor], lr: float,
               beta1: float, beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float = 1.0) -> None:
    """One AdamW step on a flat shard: master / m / v fp32 (in place), grad any of fp32 / bf16 / fp16, param_out 16-bit or fp32 or None."""
    for t, n in ((master, "master"), (m, "m"), (v, "v")):
        _chk(t, n, torch.float32)
    if not grad.is_cuda or grad.dtype not in DT_CODE or not grad.is_contiguous() or grad.numel() != master.numel():
        raise RuntimeError("u-llava_amd.adamw_step: grad must be a contiguous GPU tensor of the shard's size (fp32 / bf16 / fp16)")
    pd = 0
    if param_out is not None:
        if not param_out.is_cuda or param_out.dtype not in DT_CODE or not param_out.is_contiguous() or param_out.numel() != master.numel():
            raise RuntimeError("u-llava_amd.adamw_step: param_out must be a contiguous GPU tensor of the shard's size")
        pd = DT_CODE[param_out.dtype]
    _lib.call("ull_adamw_step_f32", _p(master), _p(m), _p(v), _p(grad), DT_CODE[grad.dtype], _p(param_out), pd, master.numel(), float(lr), float(beta1),
              float(beta2), float(eps), float(weight_decay), int(step), float(grad_scale), _stream())


def sumsq(g: torch.Tensor, out: torch.Tensor) -> None:
    """out[0] (fp32) += sum of squares of g."""
    _chk(out, "out", torch.float32)
    if not g.is_cuda or g.dtype not in DT_CODE or not g.is_contiguous():
        raise RuntimeError("u-llava_amd.sumsq: contiguous GPU tensor (fp32 / bf16 / fp16) required")
    if g.numel():
        _lib.call("ull_sumsq_f32", _p(g), DT_CODE[g.dtype], g.numel(), _p(out), _stream())


# ---- coarse entries (include/ullava_hip.h "coarse entries", csrc/layers.hip): one C call enqueues a whole stack of layers ---------------------
# The per-op wrappers above cost a ctypes round trip + Python marshalling per LAUNCH (~15 us); a C4 step has ~400 launches, a decode step ~160.
# A LayerStack holds the ctypes array of per-layer structs (weight / bias / norm pointers) and refreshes it when a pointer it recorded has
# moved (a re-made tile-major copy after an optimizer step, a re-pack).  Results are bit-identical to the per-op path: same entries, and
# the one dispatch rule (csrc/linear_route.h), which layers.hip applies directly and `_linear_route` / `_gemm_plan` read from the library.
COARSE = [True]     # `with ops.per_op_layers():` = the per-op path (tests A/B the two)


class per_op_layers:
    def __init__(self, on: bool = True):
        self.on = on

    def __enter__(self):
        self.prev = COARSE[0]
        COARSE[0] = not self.on
        return self

    def __exit__(self, *exc):
        COARSE[0] = self.prev
        return False


def coarse_ok() -> bool:
    return COARSE[0] and not _SMALL_M_SPLIT_K[0]


class LayerStack:
    """`kind`: _lib.LlamaLayer / ClipLayer / SamBlock; `layers`: one dict per layer, field name -> tensor (pointer fields) or int (plain fields) or,
    for an ull_linear field, (weight, bias-or-None) or a bare weight: a 16-bit tensor or an Fp8Weight / Mxfp4Weight."""

    def __init__(self, kind, layers):
        self.kind, self.layers = kind, layers
        self.arr = (kind * len(layers))()
        lin = [(d, n) for d in layers for n, t in kind._fields_ if t is _lib.Linear]
        # the fields that hold a 16-bit weight, whose re-binding and in-place updates `refresh` follows; a quantized weight is immutable: nothing of
        # it enters the fingerprint (and no version counter is read)
        self._w16 = [(d, n) for d, n in lin if not isinstance(d[n][0] if type(d[n]) is tuple else d[n], QuantWeight)]
        self.quantized = len(self._w16) < len(lin)
        self._seen = None
        self.refresh()

    def _fingerprint(self):
        # (address, version) of every weight: an in-place update (optimizer step, load_state_dict) bumps the version, and only then is the
        # tile-major copy re-made (`_tiled_of`, in refresh below) -- between updates the copy's address cannot change
        fp = []
        for d, n in self._w16:
            w = d[n]
            if type(w) is tuple:
                w = w[0]
            fp += (w.data_ptr(), w._version)
        return fp

    @staticmethod
    def _linear(v):
        w, b = v if type(v) is tuple else (v, None)
        if isinstance(w, QuantWeight):
            wf, q, ldq, scales, lds = w.c_args()
            return _lib.Linear(q, None, None, w.shape[0], w.shape[1], ldq, wf, scales, lds)
        if w.dim() != 2 or w.stride(1) != 1:
            raise RuntimeError("u-llava_amd: coarse entries need row-major 2-D weights")
        wt = _tiled_of(w)
        return _lib.Linear(w.data_ptr(), None if wt is None else wt.data_ptr(), _p(b), w.shape[0], w.shape[1], w.stride(0))

    def refresh(self):
        fp = self._fingerprint()
        if fp == self._seen:
            return self.arr
        for i, d in enumerate(self.layers):
            s = self.arr[i]
            for n, t in self.kind._fields_:
                v = d[n]
                if t is _lib.Linear:
                    setattr(s, n, self._linear(v))
                elif isinstance(v, int):
                    setattr(s, n, v)
                else:
                    setattr(s, n, v.data_ptr())
        self._seen = fp
        return self.arr


def _sk_args(device):
    """(ws pointer, ws bytes, min_k) of the current stream-K policy for a coarse entry."""
    min_k = _SK_MIN_K[0]
    if min_k is None:
        return None, 0, -1
    ws = _streamk_ws(device, _stream())
    return ws.data_ptr(), ws.numel(), int(min_k)


def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def llama_prefill_layers(stack: LayerStack, x_in: torch.Tensor, x_out, rope_cos, rope_sin, key_mask, B: int, S: int, H: int, hd: int, I: int,
                         eps: float):
    """x_in [B*S, D]; x_out: list of n_layers [B*S, D] tensors (may repeat; x_out[0] must not be x_in).  See ull_llama_prefill_layers_bf16."""
    _chk(x_in, "x_in")
    T, D = x_in.shape
    dev, dt = x_in.device, x_in.dtype
    x_mid = torch.empty(T, D, device=dev, dtype=dt)
    xn = torch.empty(T, D, device=dev, dtype=dt)
    qkv = torch.empty(T, 3 * D, device=dev, dtype=dt)
    att = torch.empty(T, D, device=dev, dtype=dt)
    act = torch.empty(T, I, device=dev, dtype=dt)
    ws, wsb, mk = _sk_args(dev)
    _lib.call("ull_llama_prefill_layers_" + _SFX[dt], stack.refresh(), len(stack.layers), _p(x_in), _ptr_array(x_out), _p(x_mid), _p(xn), _p(qkv), _p(att),
              _p(act), _p(rope_cos), _p(rope_sin), _p(key_mask), B, S, H, hd, I, float(eps), ws, wsb, mk, _zeros(dev).data_ptr(), _stream())


def llama_decode_layers(stack: LayerStack, x_in: torch.Tensor, x_out, rope_cos, rope_sin, key_mask, k_ptrs, vt_ptrs, B: int, S: int, H: int, hd: int,
                        I: int, smax: int, past: int, eps: float, kv8=None):
    """One generation step through all layers (T = B*S <= 4).  k_ptrs / vt_ptrs: ctypes void* arrays of the per-layer caches.  The stack's
    Linears may be quantized (bf16 activations).  kv8 = (k8, vt8, k_scale, vt_scale pointer arrays, k_stage, vt_stage) of an fp8 cache
    (KVCache.c_ptrs): ull_llama_decode_layers_kv8_bf16, k_ptrs / vt_ptrs unused."""
    _chk(x_in, "x_in", BF16 if (stack.quantized or kv8 is not None) else None)
    T, D = x_in.shape
    dev, dt = x_in.device, x_in.dtype
    scratch = torch.empty(T * (4 * D + 2 * max(D, I)), device=dev, dtype=dt)
    x_mid, q, att = scratch[:T * D], scratch[T * D:2 * T * D], scratch[2 * T * D:3 * T * D]
    xn = scratch[3 * T * D:3 * T * D + T * max(D, I)]
    act = scratch[3 * T * D + T * max(D, I):3 * T * D + T * max(D, I) + T * I]
    if kv8 is not None:
        k8, vt8, ks, vs, k_stage, vt_stage = kv8
        _lib.call("ull_llama_decode_layers_kv8_bf16", stack.refresh(), len(stack.layers), _p(x_in), _ptr_array(x_out),
                  _p(x_mid), _p(xn), _p(q), _p(att), _p(act), _p(rope_cos), _p(rope_sin), _p(key_mask), k8, vt8, ks, vs, _p(k_stage), _p(vt_stage),
                  B, S, H, hd, I, smax, past, float(eps), _zeros(dev).data_ptr(), _stream())
        return
    _lib.call("ull_llama_decode_layers_" + _SFX[dt], stack.refresh(), len(stack.layers), _p(x_in), _ptr_array(x_out), _p(x_mid),
              _p(xn), _p(q), _p(att), _p(act), _p(rope_cos), _p(rope_sin), _p(key_mask), k_ptrs, vt_ptrs, B, S, H, hd, I, smax, past, float(eps),
              _zeros(dev).data_ptr(), _stream())


def clip_layers(stack: LayerStack, n_layers: int, h: torch.Tensor, n_img: int, S: int, H: int, hd: int, I: int, eps: float):
    """The first n_layers CLIP encoder layers on h [n_img*S, D], in place."""
    _chk(h, "h")
    T, D = h.shape
    dev, dt = h.device, h.dtype
    h_mid = torch.empty(T, D, device=dev, dtype=dt)
    y = torch.empty(T, D, device=dev, dtype=dt)
    qkv = torch.empty(T, 3 * D, device=dev, dtype=dt)
    att = torch.empty(T, D, device=dev, dtype=dt)
    f = torch.empty(T, I, device=dev, dtype=dt)
    ws, wsb, mk = _sk_args(dev)
    _lib.call("ull_clip_layers_" + _SFX[dt], stack.refresh(), n_layers, _p(h), _p(h_mid), _p(y), _p(qkv), _p(att), _p(f), n_img, S, H, hd, I, float(eps),
              ws, wsb, mk, _zeros(dev).data_ptr(), _stream())


def sam_blocks(stack: LayerStack, x: torch.Tensor, B: int, g: int, nH: int, hd: int, I: int, eps: float = 1e-6):
    """All SAM encoder blocks on image-order tokens x [B*g*g, C], in place."""
    _chk(x, "x")
    T, C = x.shape
    dev, dt = x.device, x.dtype
    x_mid = torch.empty(T, C, device=dev, dtype=dt)
    y = torch.empty(T, C, device=dev, dtype=dt)
    qkv = torch.empty(T, 3 * C, device=dev, dtype=dt)
    att = torch.empty(T, C, device=dev, dtype=dt)
    f = torch.empty(T, I, device=dev, dtype=dt)
    ws, wsb, mk = _sk_args(dev)
    _lib.call("ull_sam_blocks_" + _SFX[dt], stack.refresh(), len(stack.layers), _p(x), _p(x_mid), _p(y), _p(qkv), _p(att), _p(f), B, g, nH, hd, I, float(eps),
              ws, wsb, mk, _zeros(dev).data_ptr(), _stream())
