"""No GPU: the opt-in FP8 (W8A8) Linears of the SAM image encoder (UllavaForCausalLM.set_sam_precision("fp8_e4m3"), DESIGN f12) -- the two
exported entries and their refusals, and the validation of the switch.  The GPU tests are in tests/test_sam_fp8_gpu.py."""
import os
import re

import pytest
import torch

from helpers import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMQ, GEMM = "ull_layernorm_quantize_rows_fp8_bf16", "ull_gemm_a8w8_epi_bf16"


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------
def test_header_and_library_export_both_entries_without_an_f16_twin():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    L = pkg("_lib")
    lib = L.load()
    for entry, nargs in ((NORMQ, 11), (GEMM, 16)):
        assert re.search(r"^int " + entry + r"\(", header, flags=re.M), entry
        assert entry in L.SIGNATURES and hasattr(lib, entry), entry
        params = re.search(r"^int " + entry + r"\(([^;]*)\);", header, flags=re.M | re.S).group(1)
        assert len(params.split(",")) == len(L.SIGNATURES[entry]) == nargs, entry
        twin = entry[:-4] + "f16"
        assert twin not in header and twin not in L.SIGNATURES and not hasattr(lib, twin), "fp8 activations are a bf16-only feature"
    declared = set(re.findall(r"\bint(?:64_t)? (ull_[a-z0-9_]+)\(", header))
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)


_ADDR = 0x10000                 # a non-null, 16-byte aligned address that is never dereferenced: every call returns from its argument checks
ERR_ARG, ERR_SHAPE = -1, -2


def _rc(Xq=_ADDR, ldxq=128, xs=_ADDR, Q=_ADDR, ldq=128, ws=_ADDR, bias=_ADDR, C=_ADDR, ldc=64, R=None, ldr=0, M=16, N=64, K=128, flags=0):
    return getattr(pkg("_lib").load(), GEMM)(Xq, ldxq, xs, Q, ldq, ws, bias, C, ldc, R, ldr, M, N, K, flags, None)


def test_gemm_entry_refuses_bad_arguments_without_launching():
    ops = pkg("ops")
    for null in ("Xq", "xs", "Q", "ws", "C"):
        assert _rc(**{null: None}) == ERR_ARG, null
    assert _rc(M=0) == ERR_ARG and _rc(N=0) == ERR_ARG and _rc(K=0) == ERR_ARG
    assert _rc(flags=ops.EPI_BIAS, bias=None) == ERR_ARG, "bias flag without a bias"
    assert _rc(flags=ops.EPI_RESID) == ERR_ARG, "residual flag without a residual"
    for bad in (ops.EPI_W_TILED, 128, ops.EPI_BIAS_ROUNDED, ops.EPI_BIAS | ops.EPI_BIAS_ROUNDED, 1 << 20):
        assert _rc(flags=bad) == ERR_ARG, f"flag {bad} is not part of the contract"
    for sw in (ops.EPI_BIAS, ops.EPI_GELU, ops.EPI_QGELU, ops.EPI_RELU):
        assert _rc(flags=ops.EPI_SWIGLU | sw) == ERR_SHAPE, "SwiGLU with a bias or an activation stays refused"
    assert _rc(flags=ops.EPI_SWIGLU, N=48) == ERR_SHAPE, "SwiGLU needs whole 32-row gate|up groups"
    assert _rc(K=192, ldxq=192, ldq=192) == ERR_SHAPE, "K must be a multiple of 128"
    assert _rc(K=64, ldxq=64, ldq=64) == ERR_SHAPE
    assert _rc(ldxq=129) == ERR_SHAPE and _rc(ldq=129) == ERR_SHAPE, "an odd row pitch"
    assert _rc(ldxq=136) == ERR_SHAPE and _rc(ldq=136) == ERR_SHAPE, "row pitches are multiples of 16 bytes"
    assert _rc(ldxq=112) == ERR_SHAPE and _rc(ldq=112) == ERR_SHAPE, "a row pitch below K"
    assert _rc(Xq=_ADDR + 8) == ERR_SHAPE and _rc(Q=_ADDR + 4) == ERR_SHAPE, "16-byte aligned codes"
    assert _rc(ldc=63) == ERR_SHAPE and _rc(flags=ops.EPI_RESID, R=_ADDR, ldr=8) == ERR_SHAPE, "output / residual rows shorter than N"
    # the flags the entry adds pass its checks: what is left to refuse is the shape
    for ok in (ops.EPI_BIAS, ops.EPI_BIAS | ops.EPI_GELU, ops.EPI_BIAS | ops.EPI_QGELU, ops.EPI_RELU, ops.EPI_BIAS | ops.EPI_F32):
        assert _rc(flags=ok, K=192, ldxq=192, ldq=192) == ERR_SHAPE, ok


def _rcn(X=_ADDR, ldx=128, w=_ADDR, b=_ADDR, eps=1e-6, M=4, K=128, codes=_ADDR, ldq=128, scales=_ADDR):
    return getattr(pkg("_lib").load(), NORMQ)(X, ldx, w, b, eps, M, K, codes, ldq, scales, None)


def test_norm_quantize_entry_refuses_bad_arguments_without_launching():
    for null in ("X", "w", "b", "codes", "scales"):
        assert _rcn(**{null: None}) == ERR_ARG, null
    assert _rcn(M=0) == ERR_ARG and _rcn(K=0) == ERR_ARG
    assert _rcn(K=124, ldx=128) == ERR_SHAPE, "K must be a multiple of 8"
    assert _rcn(K=8200, ldx=8200, ldq=8200) == ERR_SHAPE, "rows wider than ull_layernorm_bf16 takes"
    assert _rcn(ldx=129) == ERR_SHAPE and _rcn(ldq=129) == ERR_SHAPE, "an odd row pitch"
    assert _rcn(ldx=120) == ERR_SHAPE and _rcn(ldq=120) == ERR_SHAPE, "a row pitch below K"
    assert _rcn(X=_ADDR + 2) == ERR_SHAPE and _rcn(w=_ADDR + 8) == ERR_SHAPE and _rcn(b=_ADDR + 8) == ERR_SHAPE, "16-byte aligned rows"
    assert _rcn(codes=_ADDR + 4) == ERR_SHAPE, "8-byte aligned codes"


# ---- the switch ---------------------------------------------------------------------------------------------------------------------------
def _tiny_model(dtype=torch.bfloat16):
    C, M = pkg("configuration"), pkg("modeling_ullava")
    cfg = C.UllavaConfig(llm_config=dict(vision_config=dict(hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64, image_size=28,
                                                            patch_size=14), vocab_size=120, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                                         num_attention_heads=4), seg_token_idx=101, loc_token_idx=102, out_dim=256,
                         sam_config=dict(embed_dim=32, depth=2, num_heads=2, global_attn_indexes=[1]))
    return M.UllavaForCausalLM(cfg, dtype=dtype)


def test_mode_validation_on_a_tiny_model():
    S = pkg("sam")
    m = _tiny_model()
    assert m.sam_precision is None and m._sam.linear_precision is None and S.SamEngine.linear_precision is None
    assert S.SamEngine.LINEAR_PRECISIONS == (None, "fp8_e4m3")
    for bad in ("fp8", "FP8_E4M3", "fp8_e5m2", "mxfp4", "", 8, "bf16"):
        with pytest.raises(ValueError, match="sam precision"):
            m.set_sam_precision(bad)
        assert m.sam_precision is None, "a refused mode changes nothing"
    assert m.set_sam_precision("fp8_e4m3") is m
    assert m.sam_precision == "fp8_e4m3" and m._sam.linear_precision == "fp8_e4m3"
    assert _tiny_model().sam_precision is None, "the mode belongs to one model"
    assert m.set_sam_attention("exact") is m and m.sam_precision == "fp8_e4m3" and m.sam_attention == "exact", "the two switches are independent"
    assert m.set_sam_precision(None) is m and m.sam_precision is None and m.sam_attention == "exact"
    # an engine whose attribute was set to nonsense directly refuses to encode (before it touches the GPU)
    m._sam.linear_precision = "fp4"
    with pytest.raises(ValueError, match="linear_precision"):
        m._sam.encode(torch.zeros(1, 3, 1024, 1024, dtype=torch.bfloat16))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_other_dtypes_are_refused_by_name(dtype):
    m = _tiny_model(dtype)
    with pytest.raises(NotImplementedError, match=str(dtype).replace(".", r"\.")):
        m.set_sam_precision("fp8_e4m3")
    assert m.sam_precision is None
    assert m.set_sam_precision(None) is m, "switching off is always allowed"
    # ... and the engine itself refuses before any device work (the pixel tensor is on the CPU: a launch would raise something else)
    m._sam.linear_precision = "fp8_e4m3"
    with pytest.raises(NotImplementedError, match=str(dtype).replace(".", r"\.")):
        m._sam.encode(torch.zeros(1, 3, 1024, 1024, dtype=dtype))


def test_llm_quantization_leaves_the_sam_precision_alone(monkeypatch):
    m = _tiny_model()
    seen = []
    monkeypatch.setattr(type(m.llm), "quantize_weights", lambda self, fmt, **kw: seen.append((fmt, kw)))
    assert m.quantize_weights("fp8_e4m3", activations="fp8_e4m3") is m and len(seen) == 1
    assert m.sam_precision is None
    m.set_sam_precision("fp8_e4m3")
    m.quantize_weights("mxfp4")
    assert m.sam_precision == "fp8_e4m3" and len(seen) == 2
