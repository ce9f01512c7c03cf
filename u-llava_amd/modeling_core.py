"""UllavaCoreForCausalLM on MI355X: CLIP ViT-L -> vision_projector -> LLaMA -> lm_head.

Host-side mirror of reference `models/ullava_core.py:78-395` (same constructor, attribute names, state-dict keys,
`forward` / `encode_image` / `encode_video` / `embed_images_videos` / `prepare_inputs_for_generation` / `generate`
signatures and outputs).  The module tree exists to carry the reference's parameter names; no nn.Module.forward
of a leaf is ever used: every arithmetic op is a HIP kernel reached through `ops.py` -> C-ABI.

MI355X-specific host design:
  * weights are re-laid out once (`pack_weights`): q|k|v fused into one [3D, D] matrix (one GEMM, one pass over
    the activations), gate/up interleaved in 16-row groups so SwiGLU is a register-level GEMM epilogue, the CLIP
    patch conv flattened and K-padded to a multiple of 64 for the MFMA GEMM;
  * the residual stream is a flat [B*S, D] bf16 matrix; q/k are consumed in place from the fused QKV buffer by
    strides, V is written once as V^T (K-contiguous for the P*V MFMA);
  * the per-sample python splice loop of the reference (with its device->host syncs) is one gather kernel.
"""
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib
from . import autograd_ops as A
from . import ops
from .configuration import UllavaCoreConfig
# (imported by name: the cache and the decoding helpers stay importable from this module)
from .generation import (Decoding, GenerateOutput, beam_loop, beam_search_reference, check_generate_args, check_ngram_ban, check_prompt_lookup, check_sampler, check_stop_strings, enter_cache,
                         fused_loop, host_loop, no_repeat_ngram_banned_tokens, prompt_lookup_candidates, prompt_lookup_loop, sampling_probs, stop_strings_reference,
                         stop_table, token_byte_table)
from .kv_cache import DEFAULT_HEADROOM, KV_CACHE_DTYPES, KVCache, _check_kv_dtype

BF16 = torch.bfloat16


# ----------------------------------------------------------------------------------------------------------
# parameter holders (names match transformers' modules; forward intentionally absent)
# ----------------------------------------------------------------------------------------------------------
def _param(*shape, device=None, dtype=BF16):
    return nn.Parameter(torch.empty(*shape, device=device, dtype=dtype), requires_grad=False)



def _clear_transposes():
    from .autograd_ops import clear_transpose_cache
    clear_transpose_cache()


_ALIAS_WARNED = [False]


def _warn_alias_fallback(why: str) -> None:
    """one line, once per process: the training path fell back from aliased q|k|v / gate|up buffers to a per-step torch.cat (correct, slower)."""
    if not _ALIAS_WARNED[0]:
        _ALIAS_WARNED[0] = True
        import warnings
        warnings.warn("u-llava_amd: training forward concatenates q|k|v / gate|up under autograd on every step instead of aliasing them: " + why +
                      ".  Results are identical; call model._apply(lambda t: t) (or .to(device)) after taking ownership back to re-enable aliasing.",
                      RuntimeWarning, stacklevel=3)


def _dealias_state_dict(module, state_dict, prefix, local_metadata):
    """state-dict hook: the training path makes q|k|v and gate|up row slices of one buffer each (_alias_pack); a state dict must hold
    tensors that own their storage (safetensors refuses shared memory; HF Trainer._save writes state_dict() as it is)."""
    for k in list(state_dict.keys()):
        v = state_dict[k]
        if isinstance(v, nn.Parameter):
            continue                 # state_dict(keep_vars=True): the caller asked for the parameters themselves, aliased or not
        if k.startswith(prefix) and isinstance(v, torch.Tensor) and v.untyped_storage().nbytes() > v.numel() * v.element_size() + 64:
            state_dict[k] = v.clone()
    return state_dict


class Linear(nn.Linear):
    """An `nn.Linear` by type and by state-dict layout -- `isinstance(m, torch.nn.Linear)` is how the reference picks its LoRA targets
    (train_ullava.py:88-113 `find_linear_layers`) and how HF utilities classify parameters -- whose storage is left UNINITIALISED at
    construction (nn.Linear.__init__ would run a kaiming init over 7 B parameters on the host; weights arrive from a checkpoint or a
    seeded generator) and whose `forward` is the HIP GEMM.  The model code never calls it (the projections are operands of fused launches);
    it exists for callers that treat the module as a layer."""

    def __init__(self, in_features, out_features, bias=True, device=None, dtype=BF16):
        nn.Module.__init__(self)
        self.in_features, self.out_features = in_features, out_features
        self.weight = _param(out_features, in_features, device=device, dtype=dtype)
        if bias:
            self.bias = _param(out_features, device=device, dtype=dtype)
        else:
            self.register_parameter("bias", None)

    def reset_parameters(self) -> None:
        raise RuntimeError("u-llava_amd: parameters are loaded, never re-initialised in place")

    def forward(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad):
            return A.linear(x, self.weight, self.bias)
        return ops.linear(x, self.weight, self.bias)


class Embedding(nn.Module):
    def __init__(self, n, d, device=None, dtype=BF16):
        super().__init__()
        self.weight = _param(n, d, device=device, dtype=dtype)


class Norm(nn.Module):
    def __init__(self, d, bias=True, eps=1e-5, device=None, dtype=BF16):
        super().__init__()
        self.eps = eps
        self.weight = _param(d, device=device, dtype=dtype)
        self.bias = _param(d, device=device, dtype=dtype) if bias else None


class Conv2dHolder(nn.Module):
    def __init__(self, cin, cout, k, bias, device=None, dtype=BF16):
        super().__init__()
        self.weight = _param(cout, cin, k, k, device=device, dtype=dtype)
        self.bias = _param(cout, device=device, dtype=dtype) if bias else None


class _Holder(nn.Module):
    pass


def _llama_layer(cfg, device, dtype):
    m = _Holder()
    D, I = cfg.hidden_size, cfg.intermediate_size
    m.self_attn = _Holder()
    for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
        setattr(m.self_attn, n, Linear(D, D, bias=False, device=device, dtype=dtype))
    m.mlp = _Holder()
    m.mlp.gate_proj = Linear(D, I, bias=False, device=device, dtype=dtype)
    m.mlp.up_proj = Linear(D, I, bias=False, device=device, dtype=dtype)
    m.mlp.down_proj = Linear(I, D, bias=False, device=device, dtype=dtype)
    m.input_layernorm = Norm(D, bias=False, eps=cfg.rms_norm_eps, device=device, dtype=dtype)
    m.post_attention_layernorm = Norm(D, bias=False, eps=cfg.rms_norm_eps, device=device, dtype=dtype)
    return m


def _clip_tower(vc, device, dtype):
    D, I = vc.hidden_size, vc.intermediate_size
    m = _Holder()
    m.embeddings = _Holder()
    m.embeddings.class_embedding = _param(D, device=device, dtype=dtype)
    m.embeddings.patch_embedding = Conv2dHolder(vc.num_channels, D, vc.patch_size, bias=False, device=device, dtype=dtype)
    m.embeddings.position_embedding = Embedding((vc.image_size // vc.patch_size) ** 2 + 1, D, device=device, dtype=dtype)
    m.pre_layrnorm = Norm(D, eps=vc.layer_norm_eps, device=device, dtype=dtype)
    m.encoder = _Holder()
    layers = []
    for _ in range(vc.num_hidden_layers):
        l = _Holder()
        l.self_attn = _Holder()
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            setattr(l.self_attn, n, Linear(D, D, device=device, dtype=dtype))
        l.layer_norm1 = Norm(D, eps=vc.layer_norm_eps, device=device, dtype=dtype)
        l.mlp = _Holder()
        l.mlp.fc1 = Linear(D, I, device=device, dtype=dtype)
        l.mlp.fc2 = Linear(I, D, device=device, dtype=dtype)
        l.layer_norm2 = Norm(D, eps=vc.layer_norm_eps, device=device, dtype=dtype)
        layers.append(l)
    m.encoder.layers = nn.ModuleList(layers)
    m.post_layernorm = Norm(D, eps=vc.layer_norm_eps, device=device, dtype=dtype)
    return m


class CausalLMOutputWithPast(dict):
    """Attribute + key + index access, like transformers.modeling_outputs.CausalLMOutputWithPast."""
    _order = ("loss", "logits", "past_key_values", "hidden_states", "attentions")

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __getitem__(self, k):
        if isinstance(k, int):
            return [self.get(n) for n in self._order if self.get(n) is not None][k]
        return dict.__getitem__(self, k)


class ScoreOutput(dict):
    """What score() returns: token_logprobs, sequence_logprob, num_tokens."""
    __getattr__ = dict.__getitem__


def interleave_gate_up(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """[I, K] x2 -> [2I, K] with rows [gate 16g..16g+15 | up 16g..16g+15] per group g (ULL_EPI_SWIGLU layout)."""
    I, K = gate.shape
    assert I % 16 == 0
    return torch.stack((gate.view(I // 16, 16, K), up.view(I // 16, 16, K)), dim=1).reshape(2 * I, K).contiguous()


# ----------------------------------------------------------------------------------------------------------
class UllavaCoreForCausalLM(nn.Module):
    config_class = UllavaCoreConfig
    weight_quantization = None             # "fp8_e4m3" / "mxfp4" after quantize_weights()
    activation_quantization = None         # "fp8_e4m3" / "mxfp8_e4m3" / "mxfp4_e2m1" after quantize_weights(fmt, activations=...)
    activation_scope = "prefill"           # "prefill+decode" after quantize_weights(..., activation_scope="prefill+decode")
    decode_activation_quantization = None  # "mxfp8_e4m3" after quantize_weights("mxfp4", decode_activations="mxfp8_e4m3")

    def __init__(self, config: UllavaCoreConfig, device=None, dtype=BF16):
        super().__init__()
        if dtype not in (BF16, torch.float16, torch.float32):
            raise NotImplementedError("the MI355X path has bf16 (reference configs: bf16: true), fp16 and fp32 (inference_ullava.py --dtype "
                                      "fp16 / fp32) kernel builds")
        # (fp32: csrc/f32.hip -- plain kernels for the inference path, no fused / tiled fast paths, no backward)
        self.config = config
        D = config.hidden_size
        self.model = _Holder()
        self.model.embed_tokens = Embedding(config.vocab_size, D, device=device, dtype=dtype)
        self.model.layers = nn.ModuleList([_llama_layer(config, device, dtype) for _ in range(config.num_hidden_layers)])
        self.model.norm = Norm(D, bias=False, eps=config.rms_norm_eps, device=device, dtype=dtype)
        self.lm_head = Linear(D, config.vocab_size, bias=False, device=device, dtype=dtype)
        self.vision_encoder = _clip_tower(config.vision_config, device, dtype)
        self.vision_projector = self.build_vision_projector(config.vision_config.hidden_size, D, config.projector_type, device, dtype)
        self.vision_hidden_layer = config.vision_hidden_layer
        self.projector_from_scratch = config.projector_from_scratch
        self.mm_token_ids = config.mm_token_ids
        self.strict_checks = True          # reproduce the reference's start/end-count assert (one tiny D2H read)
        self._packed = None
        self._inv_freq = None
        self._register_state_dict_hook(_dealias_state_dict)

    # -- construction helpers ----------------------------------------------------------------------------
    @staticmethod
    def build_vision_projector(in_dim, hidden_dim, name="mlp", device=None, dtype=BF16):
        """reference models/ullava_core.py:117-129."""
        if name == "mlp":
            return Linear(in_dim, hidden_dim, device=device, dtype=dtype)
        if name == "mlp2x":
            return nn.Sequential(Linear(in_dim, hidden_dim, device=device, dtype=dtype), nn.GELU(),
                                 Linear(hidden_dim, hidden_dim, device=device, dtype=dtype))
        raise NotImplementedError

    @property
    def dtype(self):
        return self.lm_head.weight.dtype

    @property
    def device(self):
        return self.lm_head.weight.device

    def _apply(self, fn, *args, **kwargs):
        """.to() / .cuda() / .half() / .bfloat16(): the MI355X re-layouts (fused QKV, interleaved gate/up, tile-major copies) are
        derived from the parameters and are rebuilt from the moved / cast ones on the next forward."""
        if self.weight_quantization is not None:
            self._refuse_cast(fn)
            return super()._apply(fn, *args, **kwargs)
        out = super()._apply(fn, *args, **kwargs)
        self._packed = None
        _clear_transposes()          # cached W^T copies of the training path describe the old weights
        self._inv_freq = None
        self._pos_cache = None
        self._reset_alias_slots()    # every parameter is a fresh tensor: the training path may alias them anew
        return out

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def _refuse_quantized(self, what: str):
        kind = "mxfp4" if self.weight_quantization == "mxfp4" else "fp8"
        raise NotImplementedError(f"{what} is not supported on a model quantized with quantize_weights('{self.weight_quantization}'): its LLaMA "
                                  f"Linear weights exist only as {kind} codes and scales (inference only; load the bf16 model for this)")

    def _refuse_cast(self, fn):
        """_apply on a quantized model: the fp8 / mxfp4 packs are the only copy of the LLaMA weights, so a cast or a move has nothing to rebuild
        them from; a no-op (.to(the same device)) is allowed."""
        probe = torch.empty(0, device=self.device, dtype=self.dtype)
        moved = fn(probe)
        if not isinstance(moved, torch.Tensor) or moved.dtype != probe.dtype or moved.device != probe.device:
            self._refuse_quantized("changing the dtype or device (.to / .half / .float / .cpu)")

    def state_dict(self, *args, **kwargs):
        if self.weight_quantization is not None:
            self._refuse_quantized("state_dict() export")
        return super().state_dict(*args, **kwargs)

    def resize_token_embeddings(self, new_num_tokens=None, pad_to_multiple_of=None):
        """PreTrainedModel.resize_token_embeddings as the reference's callers use it (train_ullava.py:212, models/tools.py:45,72,
        102,108): grow (or shrink) embed_tokens and lm_head to `new_num_tokens` rows, old rows kept, new rows ~ N(0, 0.02)
        (LlamaPreTrainedModel._init_weights; the callers then overwrite them with the mean embedding), config.vocab_size updated."""
        emb = self.model.embed_tokens
        if new_num_tokens is None:
            return emb
        if self.weight_quantization is not None:
            self._refuse_quantized("resize_token_embeddings")
        if pad_to_multiple_of:
            new_num_tokens = -(-new_num_tokens // pad_to_multiple_of) * pad_to_multiple_of
        old = emb.weight.shape[0]
        if new_num_tokens != old:
            keep = min(old, new_num_tokens)
            for holder in (emb, self.lm_head):
                w = holder.weight
                nw = torch.empty(new_num_tokens, w.shape[1], device=w.device, dtype=w.dtype)
                nw.normal_(0.0, 0.02)
                nw[:keep] = w.data[:keep]
                holder.weight = nn.Parameter(nw, requires_grad=w.requires_grad)
            self.lm_head.out_features = new_num_tokens
            self.config.vocab_size = new_num_tokens
            self._packed = None
            _clear_transposes()          # cached W^T copies of the training path describe the old weights
        return emb

    def get_output_embeddings(self):
        return self.lm_head

    def init_mm_tokens(self, tokenizer, mm_tokens):
        ids = {k: tokenizer.convert_tokens_to_ids(v) for k, v in mm_tokens.items()}
        self.config.mm_token_ids = ids
        self.mm_token_ids = ids

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=None, device=None, **kwargs):
        """reference: inference_ullava_core.py:35 / train_ullava_core.py:94 (PreTrainedModel.from_pretrained on a local directory)."""
        from .checkpoint import core_from_pretrained
        return core_from_pretrained(cls, pretrained_model_name_or_path, torch_dtype, device, **kwargs)

    def save_pretrained(self, save_directory, **kwargs):
        if self.weight_quantization is not None:
            self._refuse_quantized("save_pretrained")
        from .checkpoint import save_pretrained
        return save_pretrained(self, save_directory, **kwargs)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        if self.weight_quantization is not None:
            self._refuse_quantized("load_state_dict")
        # transformers 4.29.1 checkpoints nest the CLIP tower under `vision_encoder.vision_model.`
        sd = {k.replace("vision_encoder.vision_model.", "vision_encoder."): v for k, v in state_dict.items()}
        sd = {k: v for k, v in sd.items() if not k.endswith("position_ids") and "rotary_emb.inv_freq" not in k}
        self._packed = None
        _clear_transposes()          # cached W^T copies of the training path describe the old weights
        return super().load_state_dict(sd, strict=strict, assign=assign)

    # -- weight re-layout ----------------------------------------------------------------------------------
    def pack_weights(self, free_originals: bool = False):
        """Build the MI355X layouts.  Call again after changing parameters."""
        if self.weight_quantization is not None:
            self._refuse_quantized("pack_weights")
        cfg = self.config
        pk = {"llama": [], "clip": []}
        lora = getattr(self, "_lora", None)

        def eff(lin):
            """the projection the inference kernels see: with an (un-merged) LoRA adapter attached, W + (alpha / r) B A rounded once --
            PeftModel.merge_adapter's arithmetic -- WITHOUT touching the parameters (generate() / evaluate() under no_grad while
            the adapters train: train_ullava.py's evaluation loop; the pack is rebuilt when the adapters change, see _pk)."""
            if lora is None or not hasattr(lin, "lora_A"):
                return lin.weight
            from .checkpoint import lora_merged_weight
            return lora_merged_weight(lin.weight, lin.lora_A.weight, lin.lora_B.weight, lora["lora_alpha"] / lora["r"])
        for l in self.model.layers:
            a, m = l.self_attn, l.mlp
            pk["llama"].append(dict(
                w_qkv=torch.cat([eff(a.q_proj), eff(a.k_proj), eff(a.v_proj)], dim=0).contiguous(),
                w_o=a.o_proj.weight, w_gu=interleave_gate_up(m.gate_proj.weight, m.up_proj.weight), w_down=m.down_proj.weight,
                ln1=l.input_layernorm.weight, ln2=l.post_attention_layernorm.weight))
        for l in self.vision_encoder.encoder.layers:
            a = l.self_attn
            pk["clip"].append(dict(
                w_qkv=torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], dim=0).contiguous(),
                b_qkv=torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], dim=0).contiguous(),
                w_out=a.out_proj.weight, b_out=a.out_proj.bias, fc1=l.mlp.fc1, fc2=l.mlp.fc2, ln1=l.layer_norm1, ln2=l.layer_norm2))
        vc = cfg.vision_config
        w = self.vision_encoder.embeddings.patch_embedding.weight
        K = vc.num_channels * vc.patch_size * vc.patch_size
        Kp = ((K + 63) // 64) * 64
        wp = torch.zeros(w.shape[0], Kp, device=w.device, dtype=w.dtype)
        wp[:, :K] = w.reshape(w.shape[0], K)
        pk["patch_w"], pk["patch_Kp"] = wp, Kp
        # fused patchify (A tiles DMA'd from the pixels): (c, ky) segments of 16, see ops.pack_patch_weight
        pk["patch_wp"] = ops.pack_patch_weight(w) if (vc.patch_size <= 16 and vc.patch_size % 2 == 0 and vc.image_size >= 16 and
                                                      w.dtype != torch.float32) else None
        # tile-major copies for the prefill-shape GEMM (+13.5 GB for LLaMA-7B; sized for 288 GB of HBM).  The row-major
        # tensors stay: they feed the decode GEMV, which streams whole rows.
        for d in pk["llama"]:
            for k in ("w_qkv", "w_o", "w_gu", "w_down"):
                ops.register_tiled(d[k])
        for d in pk["clip"]:
            for t in (d["w_qkv"], d["w_out"], d["fc1"].weight, d["fc2"].weight):
                ops.register_tiled(t)
        ops.register_tiled(self.lm_head.weight)
        pk["lora_versions"] = self._lora_versions()
        pk["llama_versions"], pk["clip_versions"] = self._llama_versions(), self._clip_versions()
        pk["freed"] = bool(free_originals)
        self._packed = pk
        if free_originals:
            for l in self.model.layers:
                for mod in (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.mlp.gate_proj, l.mlp.up_proj):
                    mod.weight.data = torch.empty(0, device=mod.weight.device, dtype=mod.weight.dtype)
        return self

    def quantize_weights(self, fmt: str = "fp8_e4m3", activations: Optional[str] = None, activation_scope: str = "prefill",
                         decode_activations: Optional[str] = None):
        """FP8 (e4m3) weight-only inference: store every LLaMA Linear (q/k/v/o/gate/up/down_proj of every layer) and lm_head as e4m3fn
        codes with one power-of-two fp32 scale per output row (ops.quantize_fp8); activations stay bf16, accumulation fp32.  Everything
        else (embeddings, norms, CLIP, projector) keeps its dtype.  Returns self.

        The result is exactly the bf16 model whose LLaMA Linear weights are replaced by dequant(codes) = float(code) * scale (a bf16 value):
        logits, hidden states and generated ids equal that twin's bit for bit.  The decode steps stream half the weight bytes (fp8 forms of
        the GEMV / skinny kernels); prefill shapes dequantize each weight into a bf16 scratch and run the bf16 GEMM.  The bf16 LLaMA
        weights and their tile-major copies are released: the fp8 packs become the only copy (like pack_weights(free_originals=True)),
        so the model can no longer train, take LoRA adapters, be saved, exported through state_dict() or cast.  bf16 models only;
        call merge_lora() first when adapters are attached.

        fmt="mxfp4": the OCP microscaling format instead (ops.quantize_mxfp4, DESIGN f7): e2m1 codes with one E8M0 power-of-two scale per row
        and block of 32 consecutive K elements, 4.25 bits per weight.  dequant = e2m1 * 2^s is a bf16 value too, so the same twin rule holds
        bit for bit, through the mxfp4 forms of the same kernels; everything said above about the fp8 model applies.  Weight-only
        round-to-nearest without calibration: the weights lose far more precision than with fp8 (profiles/mxfp4_decode.txt).  A model
        quantized to one format cannot be re-quantized to the other.

        activations="fp8_e4m3" (with fmt="fp8_e4m3" only; default None = everything above, unchanged): FP8 activations in the LLaMA prefill
        (W8A8, DESIGN f8).  Wherever the Linear dispatch rule sends one of the four LLaMA-layer Linears (q|k|v, o_proj, gate|up, down_proj) to
        the tiled GEMM -- more than 16 rows, or 5 to 16 rows against a small weight -- its input rows are quantized to e4m3 with one
        power-of-two scale per token (the weights' own rule) and the product runs on the fp8 matrix instruction from the resident codes
        (ops.linear_a8w8): no dequantized copy of the weight, twice the bf16 matrix rate.  The q|k|v projection is followed by the stand-alone
        RoPE kernel.  Decode-shape launches (GEMV / skinny) and lm_head stay W8A16, bit-identical to the weight-only model.  So this model is
        NOT the bit-exact twin of a bf16 model any more (the activations lose precision: profiles/a8w8_prefill.txt), and cached and uncached
        generation can differ: with a KV cache the prompt is prefilled in A8 and every later token is a W8A16 decode step, while
        use_cache=False re-runs the whole sequence in A8 each step.  Sample b of a batch still equals its single-sample run bit for bit
        when both run at prefill shapes.  May be called on a model that is already fp8-quantized to switch the mode on; no weight changes.
        `model.activation_quantization` reports the mode.

        activations="mxfp8_e4m3" (with fmt="mxfp4" only): MXFP8 activations in the LLaMA prefill (W4A8, DESIGN f9).  The same Linears at the
        same shapes quantize their input rows to OCP MXFP8 -- e4m3 codes with one E8M0 power-of-two scale per row and block of 32 K elements,
        the weights' own granularity -- and the product runs on the block-scaled matrix instruction straight from the resident MXFP4 codes
        and scale bytes (ops.linear_w4a8): no dequantized copy, no second weight copy.  Everything said about the fp8 mode holds with W4A16
        for W8A16 (profiles/w4a8_prefill.txt).  May be called on a model that is already mxfp4-quantized; no weight changes.  The spelling
        differs from "fp8_e4m3" on purpose: that value means one scale per token.

        activations="mxfp4_e2m1" (with fmt="mxfp4" only): MXFP4 activations in the LLaMA prefill (W4A4, DESIGN f19).  The same Linears at the
        same shapes quantize their input rows to OCP MXFP4 by the weights' own rule (ops.quantize_rows_mxfp4: e2m1 codes, one E8M0 scale per
        row and block of 32, round to nearest, ties to the even code) and the product runs on the block-scaled matrix instruction with e2m1
        for both operands (ops.linear_w4a4).  Prefill scope only; decode-shape launches and lm_head stay W4A16.  Round-to-nearest 4-bit
        activations without rotation or calibration are the crude form of the mode: the logits move far more than under "mxfp8_e4m3"
        (profiles/w4a4_prefill.txt); task accuracy on real checkpoints is unmeasured.  May be called on a model that is already
        mxfp4-quantized, also to switch from "mxfp8_e4m3"; no weight changes.

        activation_scope="prefill+decode" (with fmt="fp8_e4m3", activations="fp8_e4m3" only; default "prefill" = everything above, unchanged):
        FP8 activations in batched decode steps too (DESIGN f10).  Wherever the same dispatch rule (ops.linear_route) says "a8w8_skinny" -- 5 to
        32 rows against a LLaMA-sized weight -- the four layer Linears quantize their input rows per token (q|k|v and gate|up inside the RMSNorm launch they already pay,
        ops.rmsnorm_quantize_rows_fp8; o_proj and down_proj by ops.quantize_rows_fp8) and run the weight-streaming W8A8 kernel
        (ops.linear_a8w8_skinny) in place of the W8A16 skinny kernel (5 to 16 rows) or the 128 x 128 W8A8 GEMM (17 to 32 rows).  Steps of at
        most 4 tokens, lm_head and the coarse entries are untouched, so decoding at batch <= 4 is bit-identical to the weight-only model even
        under this scope.  Measured in profiles/a8_decode.txt.  May be switched on for a model that is already fp8 / A8-quantized;
        `model.activation_scope` reports the setting.

        decode_activations="mxfp8_e4m3" (with fmt="mxfp4" only, and with any of activations=None / "mxfp8_e4m3" / "mxfp4_e2m1"; default None =
        everything above, unchanged): MXFP8 activations in batched decode steps on mxfp4 weights (W4A8, DESIGN f20), chosen independently of the
        prefill activations -- decode is bound by the weight stream, so 4-bit activations there would only cost accuracy.  Wherever the dispatch
        rule (ops.linear_route) says "w4a8_skinny" -- 5 to 32 rows against a LLaMA-sized weight, K a multiple of 128 -- the four layer Linears
        quantize their input rows to OCP MXFP8 (q|k|v and gate|up inside the RMSNorm launch they already pay, ops.rmsnorm_quantize_rows_mxfp8;
        o_proj and down_proj in a launch of their own) and run the weight-streaming W4A8 kernel (ops.linear_w4a8_skinny) straight from the
        resident codes and scale bytes, in place of the W4A16 skinny kernel (5 to 16 rows) or of whatever the prefill mode gives 17 to 32 rows
        (dequantize + bf16 GEMM, or the 128 x 128 W4A8 / W4A4 GEMM).  The rule goes by the row count, so a prompt of 5 to 32 tokens takes the
        route too (its q|k|v followed by the stand-alone RoPE kernel).  Steps of at most 4 tokens, lm_head, the coarse entries and every other
        shape are untouched: decoding at batch <= 4 is bit-identical to the model without the keyword, and with activations=None a prefill of
        more than 32 rows stays the bit-exact twin of the dequantized bf16 model.  This is the mxfp4 spelling of fp8's
        activation_scope="prefill+decode", which stays refused on mxfp4.  Measured in profiles/w4a8_decode.txt.  May be switched on for a model
        that is already mxfp4-quantized; no weight changes.  `model.decode_activation_quantization` reports the mode."""
        if fmt not in ("fp8_e4m3", "mxfp4"):
            raise ValueError(f"quantize_weights: unknown format {fmt!r} (supported: 'fp8_e4m3', 'mxfp4')")
        if activations not in (None, "fp8_e4m3", "mxfp8_e4m3", "mxfp4_e2m1"):
            raise ValueError(f"quantize_weights: unknown activation format {activations!r} (supported: None, 'fp8_e4m3', 'mxfp8_e4m3', "
                             "'mxfp4_e2m1')")
        if activation_scope not in ("prefill", "prefill+decode"):
            raise ValueError(f"quantize_weights: unknown activation scope {activation_scope!r} (supported: 'prefill', 'prefill+decode')")
        if decode_activations not in (None, "mxfp8_e4m3"):
            raise ValueError(f"quantize_weights: unknown decode activation format {decode_activations!r} (supported: None, 'mxfp8_e4m3')")
        mx = fmt == "mxfp4"
        if decode_activations is not None and not mx:
            raise ValueError("quantize_weights('fp8_e4m3', decode_activations=...): decode_activations is the mxfp4 spelling; fp8_e4m3 weights "
                             "take activations='fp8_e4m3', activation_scope=\"prefill+decode\"")
        if activation_scope == "prefill+decode":
            if mx:
                raise NotImplementedError("quantize_weights('mxfp4', activation_scope='prefill+decode'): the scope is fp8_e4m3's spelling (one "
                                          "scale per token); mxfp4 weights take decode_activations='mxfp8_e4m3'")
            if activations is None:
                raise ValueError("quantize_weights: activation_scope='prefill+decode' needs activations='fp8_e4m3'")
        if activations == "fp8_e4m3" and mx:
            raise NotImplementedError("quantize_weights('mxfp4', activations='fp8_e4m3'): per-token fp8 activations are implemented on fp8_e4m3 "
                                      "weights only; mxfp4 weights take block-scaled activations, activations='mxfp8_e4m3'")
        if activations == "mxfp8_e4m3" and not mx:
            raise NotImplementedError("quantize_weights('fp8_e4m3', activations='mxfp8_e4m3'): block-scaled fp8 activations are implemented on "
                                      "mxfp4 weights only; fp8_e4m3 weights take activations='fp8_e4m3'")
        if activations == "mxfp4_e2m1" and not mx:
            raise NotImplementedError("quantize_weights('fp8_e4m3', activations='mxfp4_e2m1'): MXFP4 activations are implemented on mxfp4 weights "
                                      "only; fp8_e4m3 weights take activations='fp8_e4m3'")
        if activations in ("mxfp8_e4m3", "mxfp4_e2m1") or decode_activations is not None:  # (refused before any device work: the W4A8 / W4A4 kernels walk K in 128-code tiles; smaller K is padded)
            cfg_ = self.config
            for k_ in (cfg_.hidden_size, cfg_.intermediate_size):
                if k_ % 32 == 0 and not ops.w4a8_k_ok(k_):
                    mode_ = f"activations='{activations}'" if activations is not None else f"decode_activations='{decode_activations}'"
                    raise NotImplementedError(f"quantize_weights('mxfp4', {mode_}): K = {k_} is not a multiple of 128 and cannot "
                                              "be padded (the resident layout of its first 2048 elements would change)")
        if self.weight_quantization is not None:
            if self.weight_quantization == fmt:
                if activations is not None:
                    self.activation_quantization = activations
                if activation_scope != "prefill":
                    self.activation_scope = activation_scope
                if decode_activations is not None:
                    self.decode_activation_quantization = decode_activations
                return self
            self._refuse_quantized(f"quantize_weights({fmt!r})")
        if self.dtype != BF16:
            raise NotImplementedError(f"quantize_weights('{fmt}') covers bf16 models only (this one is {self.dtype}): for fp16 the dequantized "
                                      f"weights are not always representable, and fp32 has no {'mxfp4' if mx else 'fp8'} kernels")
        if getattr(self, "_lora", None) is not None:
            raise NotImplementedError("quantize_weights: LoRA adapters are attached -- call merge_lora() first")
        cfg = self.config
        bad_k = cfg.hidden_size % 32 or cfg.intermediate_size % 32
        if mx and bad_k:                     # (mxfp4 refuses before any device work: one scale per 32 elements of K)
            raise NotImplementedError("quantize_weights('mxfp4'): hidden_size and intermediate_size (the K of every LLaMA Linear) must be multiples "
                                      f"of 32 (got {cfg.hidden_size} and {cfg.intermediate_size})")
        if not self.lm_head.weight.is_cuda:
            raise RuntimeError("quantize_weights: move the model to the GPU first (the quantization runs there)")
        if bad_k:                            # (fp8: the order and the message it has always had)
            raise NotImplementedError("quantize_weights: hidden_size and intermediate_size must be multiples of 32")
        # built outside inference mode: the packs are ordinary tensors whatever mode the caller is in (and no version counter is read)
        with torch.inference_mode(False), torch.no_grad():
            pk = self._pk(for_llama=True)
            dev = self.lm_head.weight.device

            def quant(w):
                return (ops.quantize_mxfp4 if mx else ops.quantize_fp8)(w.detach().contiguous())

            def cat(qs):
                if mx:                       # (the resident layout permutes bytes within a row only: rows concatenate as they are)
                    return ops.Mxfp4Weight(torch.cat([q.codes for q in qs]), torch.cat([q.scales for q in qs]), qs[0].K)
                return ops.Fp8Weight(torch.cat([q.codes for q in qs]), torch.cat([q.scales for q in qs]))

            llama = []
            for l, d in zip(self.model.layers, pk["llama"]):
                a, m = l.self_attn, l.mlp
                # per-row scales: quantizing the q|k|v concatenation / the gate|up interleave row by row equals concatenating /
                # interleaving the per-Linear codes and scales; after pack_weights(free_originals=True) only the packs are left
                qkv = cat([quant(a.q_proj.weight), quant(a.k_proj.weight), quant(a.v_proj.weight)]) if a.q_proj.weight.numel() else quant(d["w_qkv"])
                if m.gate_proj.weight.numel():
                    g, u = quant(m.gate_proj.weight), quant(m.up_proj.weight)
                    if mx:
                        gu = ops.Mxfp4Weight(interleave_gate_up(g.codes, u.codes), interleave_gate_up(g.scales, u.scales), g.K)
                    else:
                        gu = ops.Fp8Weight(interleave_gate_up(g.codes, u.codes), interleave_gate_up(g.scales[:, None], u.scales[:, None]).view(-1))
                else:
                    gu = quant(d["w_gu"])
                llama.append(dict(w_qkv=qkv, w_o=quant(d["w_o"]), w_gu=gu, w_down=quant(d["w_down"]), ln1=d["ln1"], ln2=d["ln2"]))
            lm_head = quant(self.lm_head.weight)
            # release the bf16 LLaMA weights and every copy derived from them (packs, tile-major copies, training-path buffers)
            for d in pk["llama"]:
                for k in ("w_qkv", "w_o", "w_gu", "w_down"):
                    ops.unregister_tiled(d[k])
            mods = [self.lm_head] + [mod for l in self.model.layers for mod in (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj,
                                                                                  l.self_attn.o_proj, l.mlp.gate_proj, l.mlp.up_proj, l.mlp.down_proj)]
            for mod in mods:
                ops.unregister_tiled(mod.weight)
                mod.weight.data = torch.empty(0, device=dev, dtype=BF16)
                mod.weight.requires_grad_(False)
            new = {k: v for k, v in pk.items() if k not in ("llama", "_c_llama")}
            new.update(llama=llama, lm_head=lm_head, freed=True, fp8=not mx, mxfp4=mx)
            self._packed = None
            pk.clear()
            self._packed = new
            self._reset_alias_slots()
            _clear_transposes()
        self.weight_quantization = fmt
        self.activation_quantization = activations
        self.activation_scope = activation_scope
        self.decode_activation_quantization = decode_activations
        return self

    # The version tuples are read on EVERY forward (a decode step too): walking the module tree for them cost 0.5 ms of host time per step
    # (nn.Module.__getattr__ is Python).  The tensors are collected once per pack -- whatever re-binds a parameter (`_apply`, load_state_dict,
    # add_lora / merge_lora) also drops the pack, and with it these lists.
    def _ver_tensors(self, which: str):
        cache = self.__dict__.setdefault("_ver_cache", {})
        pk = self._packed
        if cache.get("pack") is not pk or pk is None:
            cache.clear()
            cache["pack"] = pk
        lst = cache.get(which)
        if lst is None:
            if which == "lora":
                lst = [p_ for l in self.model.layers for t in ("q_proj", "k_proj", "v_proj") if hasattr(getattr(l.self_attn, t), "lora_A")
                       for p_ in (getattr(l.self_attn, t).lora_A.weight, getattr(l.self_attn, t).lora_B.weight)]
            elif which == "llama":
                lst = [getattr(h, n).weight for l in self.model.layers
                       for h, ns in ((l.self_attn, ("q_proj", "k_proj", "v_proj")), (l.mlp, ("gate_proj", "up_proj"))) for n in ns]
            else:
                ve = self.vision_encoder
                lst = [ve.embeddings.patch_embedding.weight] + [p_ for l in ve.encoder.layers for n in ("q_proj", "k_proj", "v_proj")
                                                                  for p_ in (getattr(l.self_attn, n).weight, getattr(l.self_attn, n).bias)]
            if pk is not None:
                cache[which] = lst
        return lst

    def _lora_versions(self):
        if getattr(self, "_lora", None) is None:
            return None
        return tuple(p_._version for p_ in self._ver_tensors("lora"))

    def _llama_versions(self):
        """version counters of the LLaMA weights the packs hold COPIES of (q|k|v concatenated, gate|up interleaved)."""
        return tuple(p_._version for p_ in self._ver_tensors("llama"))

    def _clip_versions(self):
        return tuple(p_._version for p_ in self._ver_tensors("clip"))

    def _pk(self, for_llama: bool = False):
        """The packed weights, re-made when a parameter they were copied from has been written since (`._version`: an optimizer step's
        in-place update, load_state_dict, merge_lora ...).  for_llama (the inference LLaMA path) also checks the LLaMA packs: the q|k|v
        concatenations / gate|up interleaves of the base weights, and with un-merged LoRA adapters attached the adapters too (the packs
        then hold W + s B A).  The CLIP tower asks without that check: a TRAINING forward needs only the CLIP packs (its LLaMA half reads
        the parameters through _alias_pack), and re-packing 13.5 GB of LLaMA weights on every step because the parameters moved cost
        94 ms of device copies per step (profile of bench.py --workload train --train-config lora)."""
        pk = self._packed
        if pk is None:
            return self.pack_weights()._packed
        if pk.get("freed"):
            return pk                        # pack_weights(free_originals=True): the packs are the only copy, nothing to compare with
        if pk["clip_versions"] != self._clip_versions() or (for_llama and (
                pk["llama_versions"] != self._llama_versions() or pk.get("lora_versions") != self._lora_versions())):
            self.pack_weights()
        return self._packed

    # -- CLIP ----------------------------------------------------------------------------------------------
    def _selected_layer_count(self) -> int:
        L = self.config.vision_config.num_hidden_layers
        idx = self.vision_hidden_layer if self.vision_hidden_layer >= 0 else L + 1 + self.vision_hidden_layer
        if not 0 <= idx <= L:
            raise ValueError("vision_hidden_layer out of range")
        return idx          # hidden_states[idx] = output after `idx` encoder layers

    def _clip_hidden(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """hidden_states[vision_hidden_layer] of CLIPVisionModel, shape [n, 1 + patches, Dv] (CLS row kept).
        Layers past the selected one (and post_layernorm) are dead compute in the reference and are not run."""
        pk = self._pk()
        vc = self.config.vision_config
        ve = self.vision_encoder
        n = pixel_values.shape[0]
        if pixel_values.shape[-1] != vc.image_size or pixel_values.shape[-2] != vc.image_size:
            raise ValueError(f"Input image size ({pixel_values.shape[-2]}*{pixel_values.shape[-1]}) doesn't match model "
                             f"({vc.image_size}*{vc.image_size}).")
        x = pixel_values.to(self.dtype).contiguous()
        P = (vc.image_size // vc.patch_size) ** 2
        Dv, H = vc.hidden_size, vc.num_attention_heads
        hd = Dv // H
        if pk["patch_wp"] is not None:
            patches = ops.patchify(x, pk["patch_wp"], vc.patch_size)
        else:
            patches = ops.linear(ops.im2col(x, vc.patch_size, pk["patch_Kp"]), pk["patch_w"])
        S = P + 1
        h = ops.clip_embed_ln(patches, ve.embeddings.class_embedding, ve.embeddings.position_embedding.weight,
                              ve.pre_layrnorm.weight, ve.pre_layrnorm.bias, n, S, vc.layer_norm_eps).view(n * S, Dv)
        nsel = self._selected_layer_count()
        I = vc.intermediate_size
        coarse = ops.coarse_ok() and nsel > 0 and hd == 64 and n * S > 16 and 16 < S <= 704 and Dv % 64 == 0 and I % 64 == 0 and \
            h.dtype != torch.float32
        if coarse:
            # one C call for the tower's layers (csrc/layers.hip): the same launches as the loop below, bit-identical results
            stack = pk.get("_c_clip")
            if stack is None:
                stack = pk["_c_clip"] = ops.LayerStack(_lib.ClipLayer, [dict(ln1_w=w["ln1"].weight, ln1_b=w["ln1"].bias, ln2_w=w["ln2"].weight,
                                                                              ln2_b=w["ln2"].bias, qkv=(w["w_qkv"], w["b_qkv"]), out=(w["w_out"], w["b_out"]),
                                                                              fc1=(w["fc1"].weight, w["fc1"].bias), fc2=(w["fc2"].weight, w["fc2"].bias))
                                                                         for w in pk["clip"]])
            ops.clip_layers(stack, nsel, h, n, S, H, hd, I, vc.layer_norm_eps)
        for li in range(0 if coarse else nsel):
            w = pk["clip"][li]
            y = ops.layernorm(h, w["ln1"].weight, w["ln1"].bias, vc.layer_norm_eps)
            qkv = ops.linear(y, w["w_qkv"], w["b_qkv"])
            att = torch.empty(n * S, Dv, device=h.device, dtype=h.dtype)
            st = (S * 3 * Dv, hd, 3 * Dv)                       # V goes in as rows of the fused q|k|v buffer: no V^T pass
            ops.attention(qkv, qkv[:, Dv:], qkv[:, 2 * Dv:], att, n, H, S, S, hd, st, st, (S * Dv, hd, Dv), None, causal=False, scale_mode=1,
                          scale=hd ** -0.5, v_strides=st)
            h = ops.linear(att, w["w_out"], w["b_out"], residual=h)
            y = ops.layernorm(h, w["ln2"].weight, w["ln2"].bias, vc.layer_norm_eps)
            f = ops.linear(y, w["fc1"].weight, w["fc1"].bias, act="quick_gelu")
            h = ops.linear(f, w["fc2"].weight, w["fc2"].bias, residual=h)
        return h.view(n, S, Dv)

    def encode_image(self, image_tensors: torch.Tensor) -> torch.Tensor:
        """reference :146-158 -> [bs, num_patches, Dv] (CLS removed)."""
        return self._clip_hidden(image_tensors)[:, 1:]

    def encode_video(self, video_clip_tensors: torch.Tensor) -> torch.Tensor:
        """reference :160-180 -> [bs, n_frm + num_patches, Dv]."""
        b, c, t, hh, ww = video_clip_tensors.shape
        frames = video_clip_tensors.permute(0, 2, 1, 3, 4).reshape(b * t, c, hh, ww)
        h = self._clip_hidden(frames)                       # [b*t, P+1, Dv]
        return ops.video_pool(h, b, t, h.shape[1] - 1, tok_pitch=h.shape[1], tok_off=1)

    def _project(self, x: torch.Tensor) -> torch.Tensor:
        vp = self.vision_projector
        if self._training_graph():
            if not isinstance(vp, Linear):
                raise NotImplementedError("training path: projector_type 'mlp' (the configured type, configs/train/ullava_core.yaml:5)")
            return A.linear(x, vp.weight, vp.bias)
        if isinstance(vp, Linear):
            return ops.linear(x, vp.weight, vp.bias)
        return ops.linear(ops.linear(x, vp[0].weight, vp[0].bias, act="gelu"), vp[2].weight, vp[2].bias)

    # -- LoRA (train_ullava.py:219-237: get_peft_model(model.llm, LoraConfig(r, lora_alpha, target_modules, lora_dropout))) ---------
    def add_lora(self, r: int, lora_alpha: float = 16.0, lora_dropout: float = 0.0, target_modules=("q_proj", "v_proj")):
        """Attach LoRA adapters to the attention projections named in `target_modules` (the reference's default: q_proj, v_proj) of every
        LLaMA layer: `lora_A.weight` [r, in] (kaiming-uniform, PEFT's init), `lora_B.weight` [out, r] (zeros), the base weights and
        every other language-model weight frozen, the adapters trainable -- what get_peft_model leaves.  The forward adds
        (lora_alpha / r) * B(A(dropout(x))) to the projection as PEFT's Linear does; save_pretrained writes the adapter in PEFT's
        file layout and from_pretrained merges such files (checkpoint.merge_lora_adapter)."""
        import math
        if self.weight_quantization is not None:
            self._refuse_quantized("add_lora")
        targets = tuple(target_modules)
        if not targets or any(t not in ("q_proj", "k_proj", "v_proj") for t in targets):
            raise NotImplementedError("LoRA targets on this path: q_proj, k_proj, v_proj (the reference's configuration: q_proj, v_proj)")
        for p_ in self.model.parameters():
            p_.requires_grad = False
        for p_ in self.lm_head.parameters():
            p_.requires_grad = False
        for l in self.model.layers:
            for t in targets:
                lin = getattr(l.self_attn, t)
                dev, dt = lin.weight.device, lin.weight.dtype
                lin.lora_A, lin.lora_B = _Holder(), _Holder()
                a = torch.empty(r, lin.in_features, dtype=torch.float32)
                torch.nn.init.kaiming_uniform_(a, a=math.sqrt(5))
                lin.lora_A.weight = nn.Parameter(a.to(dt).to(dev), requires_grad=True)
                lin.lora_B.weight = nn.Parameter(torch.zeros(lin.out_features, r, dtype=dt, device=dev), requires_grad=True)
        self._lora = {"r": int(r), "lora_alpha": float(lora_alpha), "lora_dropout": float(lora_dropout), "target_modules": targets}
        self._packed = None
        return self

    def _lora_delta_operands(self, attn):
        """(A_cat [n*r, D], B_cat [3D, n*r] already scaled by lora_alpha / r) for the fused q|k|v projection of one layer: B_cat is block
        structured, so z = x A_cat^T followed by z B_cat^T adds each target's own B(A(x)) to its own third of the q|k|v row."""
        cfg = self._lora
        r, s_ = cfg["r"], cfg["lora_alpha"] / cfg["r"]
        D = self.config.hidden_size
        As, Bs = [], []
        present = [t for t in ("q_proj", "k_proj", "v_proj") if hasattr(getattr(attn, t), "lora_A")]
        for i, t in enumerate(present):
            lin = getattr(attn, t)
            As.append(lin.lora_A.weight)
            blk = torch.zeros(3 * D, r, device=lin.weight.device, dtype=lin.weight.dtype)
            off = ("q_proj", "k_proj", "v_proj").index(t) * D
            blk = torch.cat([blk[:off], lin.lora_B.weight * s_, blk[off + D:]], dim=0)      # (weight preparation; s_ = 2 in the reference's config)
            Bs.append(blk)
        # the GEMM kernels take K in 64-wide tiles: the rank axis is zero-padded here, once per operand pair, so that neither the forward
        # nor the backward GEMMs pad their activations (zero rows of A_cat / zero columns of B_cat add exact zeros)
        nr = len(present) * r
        pad = (-nr) % 64
        if pad:
            w0 = As[0]
            As.append(torch.zeros(pad, D, device=w0.device, dtype=w0.dtype))
            Bs.append(torch.zeros(3 * D, pad, device=w0.device, dtype=w0.dtype))
        return torch.cat(As, dim=0), torch.cat(Bs, dim=1)

    def merge_lora(self):
        """Fold the adapters into the base weights (PeftModel.merge_and_unload) and drop them: the inference kernels read plain weights."""
        cfg = getattr(self, "_lora", None)
        if cfg is None:
            return self
        s_ = cfg["lora_alpha"] / cfg["r"]
        from .checkpoint import lora_merged_weight
        with torch.no_grad():
            for l in self.model.layers:
                for t in cfg["target_modules"]:
                    lin = getattr(l.self_attn, t)
                    lin.weight.copy_(lora_merged_weight(lin.weight, lin.lora_A.weight, lin.lora_B.weight, s_))
                    del lin.lora_A, lin.lora_B
        self._lora = None
        self._packed = None
        _clear_transposes()
        return self

    # -- training path ---------------------------------------------------------------------------------------
    def _training_graph(self) -> bool:
        """True when this call must build an autograd graph: gradients enabled and some parameter of the language model or the
        projector asks for one (the reference freezes / unfreezes by `requires_grad`, train_ullava.py:207-261).  The CLIP tower
        is frozen by both training scripts and always runs the inference kernels without a graph."""
        if not torch.is_grad_enabled():
            return False                     # no_grad / eval with adapters attached: inference kernels on a temporarily merged pack (_pk)
        if self.dtype == torch.float32:
            # the fp32 build (csrc/f32.hip) is the INFERENCE path (`--dtype fp32` of inference_ullava.py): there are no fp32 backward kernels, so an
            # fp32 model never builds a graph -- its outputs carry no grad_fn, like the reference's under torch.inference_mode()
            return False
        if getattr(self, "_lora", None) is not None:
            return True
        return any(p.requires_grad for p in self.lm_head.parameters()) or any(p.requires_grad for p in self.model.parameters()) or \
            any(p.requires_grad for p in self.vision_projector.parameters())

    def enable_input_require_grads(self):
        """PreTrainedModel API used by train_ullava.py:214 (makes checkpointed segments differentiable in HF); the HIP training path
        needs nothing here."""
        return None

    def gradient_checkpointing_enable(self, *args, **kwargs):
        """train_ullava.py:215.  Activations are kept (288 GB of HBM per GPU): accepted and recorded, not acted upon."""
        self.config.gradient_checkpointing = True

    def gradient_checkpointing_disable(self):
        self.config.gradient_checkpointing = False

    alias_packed_weights = True          # training path: q|k|v and gate|up parameters as row slices of one buffer each (see _alias_pack)

    @staticmethod
    def _alias_pack(holder, names, slot, enabled: bool = True):
        """Make the parameters `names` of `holder` row slices of ONE [sum(N_i), K] buffer (storage shared; values, shapes, names and
        state-dict entries unchanged) and return (that buffer, the parameters).

        The aliasing is established ONCE per holder (and again after .to() / .half(), which re-create every parameter: _apply clears the
        slots) -- and only if every parameter still owns its storage at that moment.  If a parameter is a view into somebody's flat
        buffer already, or the aliasing is found broken later -- a parameter's `.data` no longer points into the buffer -- somebody else has taken
        ownership of the parameter storage (DeepSpeed ZeRO-1/2 rebinds p.data to its flat bit16 partition, FSDP to its flat parameter):
        rebinding `.data` again would detach the parameters from that owner and its updates would never be seen.  The holder is then
        marked and this function returns (None, params): the caller concatenates the live parameters under autograd instead (one
        device copy per step, always correct).  `model.alias_packed_weights = False` turns the aliasing off altogether."""
        ws = [getattr(holder, n).weight for n in names]
        if not enabled or getattr(holder, slot + "_external", False):
            return None, ws
        packed = getattr(holder, slot, None)
        if packed is not None:
            ok = packed.device == ws[0].device and packed.dtype == ws[0].dtype
            o = 0
            for w in ws:
                ok = ok and w.data_ptr() == packed.data_ptr() + o * packed.shape[1] * packed.element_size() and w.is_contiguous()
                o += w.shape[0]
            if ok and o == packed.shape[0]:
                return packed, ws
            object.__setattr__(holder, slot, None)
            object.__setattr__(holder, slot + "_external", True)          # storage re-bound by an external owner: leave it alone
            _warn_alias_fallback("the parameters no longer point into the packed buffer (an external owner re-bound their storage)")
            return None, ws
        # First call on this holder.  A parameter that is already a VIEW into a larger storage has an owner: deepspeed.initialize
        # (ZeRO-1/2: p.data = a slice of the flat bit16 group) or an FSDP wrap (flat parameter) ran before the first training forward --
        # the order HF Trainer uses.  Taking the storage away here would leave the owner updating a buffer nobody reads.
        if any(w.storage_offset() != 0 or w.untyped_storage().nbytes() > w.numel() * w.element_size() + 64 for w in ws):
            object.__setattr__(holder, slot + "_external", True)
            _warn_alias_fallback("a parameter is already a view into a larger storage (DeepSpeed / FSDP flat buffer, load_state_dict(assign=True) "
                                 "from an mmap, or a user-side flat parameter)")
            return None, ws
        with torch.no_grad():
            packed = torch.cat([w.data for w in ws], dim=0).contiguous()
            o = 0
            for w in ws:
                w.data = packed[o:o + w.shape[0]]
                o += w.shape[0]
        object.__setattr__(holder, slot, packed)             # a plain attribute: not a Parameter, not a buffer, not in the state dict
        return packed, ws

    def _reset_alias_slots(self):
        """after _apply (.to / .cuda / .half): where the move re-created the parameters the shared buffers describe dead tensors -- drop them
        (and any `external owner` mark) so that the next training forward aliases the new parameters; a no-op move keeps the aliasing."""
        for l in self.model.layers:
            for h, slot, names in ((l.self_attn, "_qkv_pack", ("q_proj", "k_proj", "v_proj")), (l.mlp, "_gu_pack", ("gate_proj", "up_proj"))):
                packed = h.__dict__.get(slot)
                if packed is not None:
                    ws, o, ok = [getattr(h, n).weight for n in names], 0, True
                    for w in ws:
                        ok = ok and w.device == packed.device and w.dtype == packed.dtype and \
                            w.data_ptr() == packed.data_ptr() + o * packed.shape[1] * packed.element_size()
                        o += w.shape[0]
                    if ok:
                        continue
                for a in (slot, slot + "_external"):
                    if a in h.__dict__:
                        object.__delattr__(h, a)

    def _llama_train(self, inputs_embeds, attention_mask, position_ids, output_hidden_states):
        """LlamaModel.forward with an autograd graph: the same HIP forward kernels (SwiGLU un-fused, RoPE stand-alone, weights
        re-packed under autograd so gradients reach q/k/v/gate/up_proj), HIP backward kernels (autograd_ops.py)."""
        cfg = self.config
        B, S, D = inputs_embeds.shape
        H = cfg.num_attention_heads
        hd = D // H
        dev = inputs_embeds.device
        if position_ids is None:
            pos = torch.arange(S, device=dev, dtype=torch.int64).repeat(B)
        else:
            pos = position_ids.to(torch.int64).expand(B, S).reshape(-1).contiguous()
        key_mask = None if attention_mask is None else attention_mask.to(torch.int32).contiguous()
        inv_freq = self._rope_inv_freq(dev)
        x = inputs_embeds.reshape(B * S, D)
        all_h = []
        for l in self.model.layers:
            if output_hidden_states:
                all_h.append(x.view(B, S, D))
            a, m = l.self_attn, l.mlp
            # q|k|v and gate|up are each ONE buffer whose row slices are the parameters (no per-step torch.cat / interleave of trainable
            # weights, one dW GEMM per pack whose row slices are the parameters' gradients)
            w_qkv, qkv_w = self._alias_pack(a, ("q_proj", "k_proj", "v_proj"), "_qkv_pack", self.alias_packed_weights)
            x, x_res = A.fork(x)                                 # two consumers: the norm and the residual add of o_proj
            h = A.rmsnorm(x, l.input_layernorm.weight, cfg.rms_norm_eps)
            # (no shared buffer -- an external owner holds the parameter storage, see _alias_pack: concatenate under autograd)
            qkv_lin = A.linear_packed(h, w_qkv, *qkv_w) if w_qkv is not None else A.linear(h, torch.cat(qkv_w, dim=0))
            if getattr(self, "_lora", None) is not None:
                # PEFT's Linear.forward: result += lora_B(lora_A(dropout(x))) * scaling -- here as two skinny GEMMs for the whole q|k|v row,
                # the base projection riding along as the second one's residual operand
                a_cat, b_cat = self._lora_delta_operands(a)
                hd_in = A.dropout(h, self._lora["lora_dropout"]) if (self.training and self._lora["lora_dropout"] > 0) else h
                qkv_lin = A.linear(A.linear(hd_in, a_cat), b_cat, residual=qkv_lin)
            qkv = A.rope(qkv_lin, pos, inv_freq, 2 * H, hd)
            att = A.self_attention(qkv, key_mask, B, S, H, hd, True)
            x = A.linear(att, a.o_proj.weight, residual=x_res)
            x, x_res = A.fork(x)
            h = A.rmsnorm(x, l.post_attention_layernorm.weight, cfg.rms_norm_eps)
            w_gu, gu_w = self._alias_pack(m, ("gate_proj", "up_proj"), "_gu_pack", self.alias_packed_weights)
            gu = A.linear_packed(h, w_gu, *gu_w) if w_gu is not None else A.linear(h, torch.cat(gu_w, dim=0))      # columns [gate | up]
            x = A.linear(A.swiglu(gu, halves=True), m.down_proj.weight, residual=x_res)
        x = A.rmsnorm(x, self.model.norm.weight, cfg.rms_norm_eps)
        last = x.view(B, S, D)
        if output_hidden_states:
            all_h.append(last)
        return last, (tuple(all_h) if output_hidden_states else None)

    # -- embedding + splice ----------------------------------------------------------------------------------
    def embed_images_videos(self, input_ids=None, images=None, videos=None):
        """reference :182-277.  Returns (input_ids, None) when S == 1, else (None, inputs_embeds [B,S,D])."""
        if input_ids.shape[1] == 1:
            return input_ids, None
        ids = input_ids.contiguous()
        mm = self.mm_token_ids
        img_feat = vid_feat = None
        img_tokens = img_pitch = img_off = 0
        if images is not None:
            with torch.no_grad():                           # the CLIP tower is frozen (train_ullava.py:207-208, ullava_core.py:148)
                h = self._clip_hidden(images)               # [n, P+1, Dv]; the projector also runs on the CLS row,
            img_feat = self._project(h.view(-1, h.shape[-1])).view(h.shape[0], h.shape[1], -1)   # which the splice skips
            img_pitch, img_off, img_tokens = h.shape[1], 1, h.shape[1] - 1
        if videos is not None:
            with torch.no_grad():
                v = self.encode_video(videos)
            vid_feat = self._project(v.view(-1, v.shape[-1])).view(v.shape[0], v.shape[1], -1)
        spans = None
        if mm is not None or self.strict_checks:
            m_ = mm or {"IMG_START": -1, "IMG_END": -1, "VID_START": -1, "VID_END": -1}
            spans = ops.mm_spans(ids, m_["IMG_START"], m_["IMG_END"], m_["VID_START"], m_["VID_END"], self.model.embed_tokens.weight.shape[0])
            if self.strict_checks:
                sp = spans.cpu()
                if int((sp[:, 3] & 2).sum()):
                    raise IndexError("index out of range in self")         # nn.Embedding on an out-of-vocabulary id
                assert int((sp[:, 3] & 1).sum()) == 0, "Number of image/video start and end tokens should be the same."
                if int((sp[:, 0] == 1).sum()) > (0 if img_feat is None else img_feat.shape[0]) or \
                        int((sp[:, 0] == 2).sum()) > (0 if vid_feat is None else vid_feat.shape[0]):
                    raise IndexError("fewer images/videos than samples that reference one")
            if mm is None:
                spans = None
        if self._training_graph():
            # projector_from_scratch (stage 1, configs/train/ullava_core.yaml): reference :230-240 detaches every text row of a
            # sample that carries an image / video except its start / end token rows
            emb = A.embed_splice(self.model.embed_tokens.weight, img_feat, vid_feat, ids, spans, img_tokens, img_pitch, img_off,
                                 detach_text=bool(self.projector_from_scratch))
        else:
            emb = ops.embed_splice(ids, self.model.embed_tokens.weight, img_feat, vid_feat, spans, img_tokens, img_pitch, img_off)
        return None, emb

    # -- LLaMA ---------------------------------------------------------------------------------------------
    def _rope_inv_freq(self, device):
        if self._inv_freq is None or self._inv_freq.device != device:
            hd = self.config.hidden_size // self.config.num_attention_heads
            inv = 1.0 / (self.config.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.float) / hd))   # LlamaRotaryEmbedding
            self._inv_freq = inv.to(device)
        return self._inv_freq

    def _pos_arange(self, device, n: int) -> torch.Tensor:
        ar = getattr(self, "_pos_cache", None)
        if ar is None or ar.device != device or ar.numel() < n:
            ar = self._pos_cache = torch.arange(max(4096, 2 * n), device=device, dtype=torch.int64)
        return ar

    def _llama(self, inputs_embeds, attention_mask, position_ids, output_hidden_states, cache: Optional[KVCache] = None):
        """LlamaModel.forward.  cache=None: plain prefill.  cache empty: prefill that also fills the cache.  cache filled:
        incremental step(s) -- the new tokens' q attend to cached K / V^T plus their own."""
        cfg = self.config
        pk = self._pk(for_llama=True)
        B, S, D = inputs_embeds.shape
        H = cfg.num_attention_heads
        hd = D // H
        dev = inputs_embeds.device
        past = cache.length if cache is not None else 0
        if position_ids is None:
            # positions past .. past + S - 1 of every row: a slice of one arange kept per device (a decode step at batch 1 then costs no
            # torch kernel for its positions -- it was an arange and an add per step; larger batches pay one repeat)
            ar = self._pos_arange(dev, past + S)
            pos = ar[past:past + S] if B == 1 else ar[past:past + S].repeat(B)
        else:
            pos = position_ids.to(torch.int64).expand(B, S).reshape(-1).contiguous()
        key_mask = None if attention_mask is None else attention_mask.to(torch.int32).contiguous()
        if cache is not None and past + S > cache.smax:
            raise RuntimeError(f"KV cache too small: {past + S} > {cache.smax}")
        inv_freq = self._rope_inv_freq(dev)
        x = inputs_embeds.reshape(B * S, D)
        T = B * S
        # prefill with LLaMA's head_dim: RoPE runs inside the QKV GEMM's epilogue from one cos / sin table per forward (the
        # positions are the same for every layer); other shapes (tiny test models, decode steps) use the stand-alone kernels
        f32 = x.dtype == torch.float32       # fp32 build: stand-alone RoPE kernels, one generic GEMM / attention (csrc/f32.hip)
        fuse_rope = hd == 128 and T > 4 and D % 64 == 0 and not (cache is not None and past > 0) and not f32
        # generation steps of at most 4 tokens (the GEMV shapes): RoPE and the cache append run in the q|k|v GEMV's epilogue, from the
        # same per-forward table
        # (that kernel stages the T x D activations in its LDS: LLaMA-7B at T = 4 is exactly the limit; wider models / more rows take the
        # stand-alone RMSNorm + RoPE-append kernels below)
        fuse_append = cache is not None and past > 0 and not f32 and ops.decode_step_fused(T, D, hd)
        wq = pk.get("fp8", False) or pk.get("mxfp4", False)      # quantize_weights(): the Linear weights are ops.Fp8Weight / ops.Mxfp4Weight
        # quantize_weights(activations=, activation_scope=): the layer Linears hand the mode to the dispatch rule (ops.linear(act_quant=))
        aq = None
        if wq and (self.activation_quantization is not None or self.decode_activation_quantization is not None):
            aq = ops.ActQuant(self.activation_quantization, self.activation_scope == "prefill+decode", self.decode_activation_quantization)
        if aq is not None and fuse_rope and pk["llama"] and ops.linear_route(T, pk["llama"][0]["w_qkv"], aq) in ops.A8_ROUTES:
            fuse_rope = False                # A8 q|k|v: the plain projection, then the stand-alone RoPE kernel
        rope_cs = ops.rope_table(pos, inv_freq, x.dtype) if (fuse_rope or fuse_append) else None
        all_h = []
        I = cfg.intermediate_size
        coarse = None
        kv8 = cache is not None and cache.kv_dtype is not None
        if kv8 and x.dtype != BF16:
            _check_kv_dtype(cache.kv_dtype, x.dtype)
        # fp8 cache, past > 0: up to 16 new tokens against more than 64 keys take the fp8 decode attention (the appenders write the
        # staging window); other calls dequantize each layer into a bf16 scratch, run the bf16 path on it and quantize the new positions back
        kv8_fewq = kv8 and past > 0 and S <= 16 and 64 < past + S <= 4096
        kv8_scr = []                          # (the per-call bf16 scratch of the other fp8-cache calls, made on first use)
        if ops.coarse_ok() and pk["llama"]:
            if fuse_append and I % 8 == 0 and (kv8_fewq or not kv8):
                coarse = "decode"
            elif fuse_rope and cache is None and T > 16 and 16 < S <= 1024 and I % 64 == 0 and not wq:
                coarse = "prefill"           # (a quantized model's prefill takes the per-op path: dequantize + GEMM per Linear)
        if coarse is not None:
            # one C call for the whole layer stack (csrc/layers.hip): the same launches as the loop below, bit-identical results
            stack = pk.get("_c_llama")
            if stack is None:
                stack = pk["_c_llama"] = ops.LayerStack(_lib.LlamaLayer, [dict(ln1=w["ln1"], ln2=w["ln2"], qkv=w["w_qkv"], o=w["w_o"], gu=w["w_gu"],
                                                                               down=w["w_down"]) for w in pk["llama"]])
            L = len(pk["llama"])
            if output_hidden_states:
                outs = [torch.empty(T, D, device=dev, dtype=x.dtype) for _ in range(L)]
                all_h = [x.view(B, S, D)] + [o.view(B, S, D) for o in outs[:-1]]
            else:
                outs = [torch.empty(T, D, device=dev, dtype=x.dtype)] * L
            if coarse == "decode" and kv8:
                ops.llama_decode_layers(stack, x, outs, rope_cs[0], rope_cs[1], key_mask, None, None, B, S, H, hd, I, cache.smax, past, cfg.rms_norm_eps,
                                        kv8=cache.c_ptrs())
            elif coarse == "decode":
                ops.llama_decode_layers(stack, x, outs, rope_cs[0], rope_cs[1], key_mask, cache.c_ptrs()[0], cache.c_ptrs()[1], B, S, H, hd, I, cache.smax,
                                        past, cfg.rms_norm_eps)
            else:
                ops.llama_prefill_layers(stack, x, outs, rope_cs[0], rope_cs[1], key_mask, B, S, H, hd, I, cfg.rms_norm_eps)
            x = outs[-1]
        for li, w in enumerate(pk["llama"] if coarse is None else ()):
            if output_hidden_states:
                all_h.append(x.view(B, S, D))
            decode = cache is not None and past > 0
            if kv8 and decode:
                kc, vtc, smax_, past_ = cache._kv8_decode_buffers(li, past, kv8_fewq, kv8_scr)
            elif decode:
                kc, vtc, smax_, past_ = cache.k[li], cache.vt[li], cache.smax, past
            if fuse_append:
                q = ops.linear_qkv_rope_append(x, w["w_qkv"], rope_cs[0], rope_cs[1], B, S, H, hd, kc, vtc, smax_, past_, rms_w=w["ln1"],
                                               rms_eps=cfg.rms_norm_eps)
                att = torch.empty(T, D, device=dev, dtype=x.dtype)
                if kv8:
                    cache._kv8_attention(q, (S * D, hd, D), li, att, B, H, S, past, hd, key_mask, kv8_fewq, kv8_scr)
                else:
                    ops.attention(q, kc, vtc, att, B, H, S, past + S, hd, (S * D, hd, D), (H * cache.smax * hd, cache.smax * hd, hd),
                                  (S * D, hd, D), key_mask, causal=True, scale_mode=1, scale=hd ** -0.5)
                x = ops.linear(att, w["w_o"], residual=x, act_quant=aq)
                a = ops.linear(x, w["w_gu"], swiglu=True, rms_w=w["ln2"], rms_eps=cfg.rms_norm_eps, act_quant=aq)
                x = ops.linear(a, w["w_down"], residual=x, act_quant=aq)
                continue
            if fuse_rope:
                qkv = ops.linear_qkv_rope(ops.rmsnorm(x, w["ln1"], cfg.rms_norm_eps), w["w_qkv"], rope_cs[0], rope_cs[1], 2 * D, hd)
            else:
                qkv = ops.linear(x, w["w_qkv"], rms_w=w["ln1"], rms_eps=cfg.rms_norm_eps, act_quant=aq)    # input_layernorm -> q|k|v
            att = torch.empty(T, D, device=dev, dtype=x.dtype)
            if decode:
                # generation step: RoPE + cache append in one launch, then the split-key attention over the cache
                ops.rope_append(qkv, 3 * D, pos, inv_freq, B, S, H, hd, kc, vtc, smax_, past_)
                if kv8:
                    cache._kv8_attention(qkv, (S * 3 * D, hd, 3 * D), li, att, B, H, S, past, hd, key_mask, kv8_fewq, kv8_scr)
                else:
                    ops.attention(qkv, kc, vtc, att, B, H, S, past + S, hd, (S * 3 * D, hd, 3 * D), (H * cache.smax * hd, cache.smax * hd, hd),
                                  (S * D, hd, D), key_mask, causal=True, scale_mode=1, scale=hd ** -0.5)
            else:
                if not fuse_rope:
                    ops.rope_inplace(qkv, 3 * D, pos, inv_freq, T, 2 * H, hd)
                st = (S * 3 * D, hd, 3 * D)
                if cache is None:                                # V goes in as rows of the fused q|k|v buffer: no V^T pass
                    ops.attention(qkv, qkv[:, D:], qkv[:, 2 * D:], att, B, H, S, S, hd, st, st, (S * D, hd, D), key_mask, causal=True,
                                  scale_mode=1, scale=hd ** -0.5, v_strides=st)
                elif kv8:                                        # prefill into an fp8 cache: the bf16-cache prefill on a transient V^T, then
                    vt = torch.empty(B, H, hd, cache.smax, device=dev, dtype=x.dtype)      # the K rows and V rows quantized into the cache
                    ops.transpose_v(qkv[:, 2 * D:], S * 3 * D, 3 * D, B, S, H, hd, pitch=cache.smax, out=vt)
                    ops.attention(qkv, qkv[:, D:], vt, att, B, H, S, S, hd, st, st, (S * D, hd, D), key_mask, causal=True, scale_mode=1,
                                  scale=hd ** -0.5)
                    ops.quantize_kv(qkv[:, D:], st, qkv[:, 2 * D:], st, *cache.kv8_layer(li), 0, S)
                else:                                            # prefill that also fills the cache (K rows, V^T image)
                    kc, vt = cache.k[li], cache.vt[li]
                    kc[:, :, :S].copy_(qkv.view(B, S, 3, H, hd)[:, :, 1].permute(0, 2, 1, 3))
                    ops.transpose_v(qkv[:, 2 * D:], S * 3 * D, 3 * D, B, S, H, hd, pitch=cache.smax, out=vt)
                    ops.attention(qkv, qkv[:, D:], vt, att, B, H, S, S, hd, st, st, (S * D, hd, D), key_mask, causal=True, scale_mode=1,
                                  scale=hd ** -0.5)
            x = ops.linear(att, w["w_o"], residual=x, act_quant=aq)
            a = ops.linear(x, w["w_gu"], swiglu=True, rms_w=w["ln2"], rms_eps=cfg.rms_norm_eps, act_quant=aq)    # post_attention_layernorm -> gate|up
            x = ops.linear(a, w["w_down"], residual=x, act_quant=aq)
        x = ops.rmsnorm(x, self.model.norm.weight, cfg.rms_norm_eps)
        last = x.view(B, S, D)
        if cache is not None:
            cache.length = past + S
            cache.last_hidden.append(last)
        if output_hidden_states:
            all_h.append(last)
        return last, (tuple(all_h) if output_hidden_states else None)

    def forward(self, input_ids: torch.LongTensor = None, attention_mask: Optional[torch.Tensor] = None,
                position_ids: Optional[torch.LongTensor] = None, past_key_values: Optional[List[torch.FloatTensor]] = None,
                inputs_embeds: Optional[torch.FloatTensor] = None, labels: Optional[torch.LongTensor] = None,
                use_cache: Optional[bool] = None, output_attentions: Optional[bool] = None,
                output_hidden_states: Optional[bool] = None, images: Optional[torch.FloatTensor] = None,
                videos: Optional[torch.FloatTensor] = None, return_dict: Optional[bool] = None):
        """reference :279-355 (same argument list)."""
        if output_attentions:
            raise NotImplementedError("attention probabilities never leave LDS on this path")
        if self.weight_quantization is not None and self._training_graph():
            self._refuse_quantized("building a training graph (gradients enabled with trainable parameters; use torch.no_grad())")
        cache = past_key_values
        if cache is not None and not isinstance(cache, KVCache):
            # an HF-style cache handed in by the caller (legacy tuple of (key, value) per layer, or a transformers Cache object)
            cache = KVCache.from_hf(cache, headroom=DEFAULT_HEADROOM)
        output_hidden_states = output_hidden_states if output_hidden_states is not None else self.config.output_hidden_states
        return_dict = return_dict if return_dict is not None else self.config.use_return_dict
        fed_ids = input_ids if inputs_embeds is None else None       # (what a cache remembers it was filled with)
        if inputs_embeds is None:
            ids, inputs_embeds = self.embed_images_videos(input_ids, images, videos)
            if inputs_embeds is None:
                inputs_embeds = ops.embed_splice(ids.contiguous(), self.model.embed_tokens.weight, None, None, None)
        if use_cache and cache is None:
            B_, S_ = inputs_embeds.shape[:2]
            cache = KVCache(self.config.num_hidden_layers, B_, self.config.num_attention_heads,
                            self.config.hidden_size // self.config.num_attention_heads,
                            max(S_ + DEFAULT_HEADROOM, 64), inputs_embeds.device, inputs_embeds.dtype)
        if self._training_graph():
            if cache is not None:
                raise NotImplementedError("use_cache / past_key_values are inference features (the training scripts set use_cache=False)")
            last, all_h = self._llama_train(inputs_embeds, attention_mask, position_ids, output_hidden_states)
            logits = A.linear(last, self.lm_head.weight)
            loss = A.shifted_cross_entropy(logits, labels) if labels is not None else None
        else:
            last, all_h = self._llama(inputs_embeds, attention_mask, position_ids, output_hidden_states, cache)
            if cache is not None:
                cache.note_fed(fed_ids, inputs_embeds.shape[1], attention_mask)
            logits = ops.linear(last, self._packed["lm_head"] if self.weight_quantization is not None else self.lm_head.weight)
            loss = ops.shifted_cross_entropy(logits, labels) if labels is not None else None
        if not return_dict:
            # reference :346-348: (loss,) + (logits,) + LlamaModel outputs[1:] = past_key_values / hidden_states when requested
            out = (logits,) + ((cache,) if cache is not None else ()) + ((all_h,) if all_h is not None else ())
            return ((loss,) + out) if loss is not None else out
        return CausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=cache, hidden_states=all_h, attentions=None)

    def prepare_inputs_for_generation(self, input_ids=None, inputs_embeds=None, attention_mask=None, images=None, videos=None,
                                      labels=None, past_key_values=None, **kwargs):
        """reference :357-395."""
        if past_key_values:
            input_ids = input_ids[:, -1:]
        position_ids = kwargs.get("position_ids", None)
        if attention_mask is not None and position_ids is None:
            position_ids = attention_mask.long().cumsum(-1) - 1
            position_ids.masked_fill_(attention_mask == 0, 1)
            if past_key_values:
                position_ids = position_ids[:, -1].unsqueeze(-1)
        model_inputs = {"inputs_embeds": inputs_embeds} if inputs_embeds is not None and past_key_values is None else {"input_ids": input_ids}
        model_inputs.update({"position_ids": position_ids, "past_key_values": past_key_values, "use_cache": kwargs.get("use_cache"),
                             "attention_mask": attention_mask, "images": images, "videos": videos})
        return model_inputs

    def new_kv_cache(self, batch_size: int, capacity: int, kv_cache_dtype=None) -> KVCache:
        """An empty KVCache of this model's geometry on its device, with room for `capacity` positions (generate() grows it when a call
        needs more): what a first generate(past_key_values=) / evaluate(past_key_values=) call fills and later calls continue."""
        cfg = self.config
        H = cfg.num_attention_heads
        return KVCache(cfg.num_hidden_layers, int(batch_size), H, cfg.hidden_size // H, max(int(capacity), 64), self.device, self.dtype,
                       kv_dtype=kv_cache_dtype)

    @torch.no_grad()
    def score(self, input_ids, attention_mask=None, images=None, videos=None, labels=None):
        """The log-probability the model gives to tokens it is handed (ranking fixed answers, scoring a caption): one forward() without a
        cache, then ops.token_logprobs per row on logits[b, :-1] against labels[b, 1:] as views -- no [B, L, V] copy, no fp32 logits.
        Returns token_logprobs fp32 [B, L-1] (column t scores token t+1 given the positions <= t; exactly 0.0 where labels[:, t+1] == -100
        or attention_mask[:, t+1] == 0), sequence_logprob [B] (the row's plain sum(-1)) and num_tokens int64 [B] (the scored positions).
        labels defaults to input_ids; pass -100 over the prompt to score only the answer (and over image / video patch positions, whose
        ids are placeholders)."""
        if not input_ids.is_cuda:
            raise RuntimeError("score() needs GPU tensors (no CPU path exists)")
        labels = input_ids if labels is None else labels
        logits = self.forward(input_ids=input_ids, attention_mask=attention_mask, images=images, videos=videos, use_cache=False,
                              return_dict=True).logits
        B, L = logits.shape[:2]
        if labels.dim() != 2 or tuple(labels.shape) != (B, L) or labels.dtype != torch.int64:
            raise ValueError(f"score(): labels must be int64 [{B}, {L}] (one per position of the forward), got {labels.dtype} {tuple(labels.shape)}")
        keep = None
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (B, L):
                raise ValueError(f"score(): attention_mask must be [{B}, {L}], got {tuple(attention_mask.shape)}")
            keep = attention_mask[:, 1:].ne(0).to(torch.int32).contiguous()
        lp = torch.zeros(B, max(L - 1, 0), dtype=torch.float32, device=logits.device)
        if L > 1:
            for b in range(B):
                ops.token_logprobs(logits[b, :-1], labels[b, 1:], None if keep is None else keep[b], out=lp[b])
        scored = (labels[:, 1:] >= 0) & (labels[:, 1:] < logits.shape[-1])
        if keep is not None:
            scored = scored & keep.bool()
        return ScoreOutput(token_logprobs=lp, sequence_logprob=lp.sum(-1), num_tokens=scored.sum(-1))

    @torch.no_grad()
    def generate(self, input_ids=None, images=None, videos=None, attention_mask=None, max_new_tokens=32, do_sample=False,
                 temperature=1.0, top_p=None, top_k=50, num_beams=1, no_repeat_ngram_size=None, stopping_criteria=None, eos_token_id=None,
                 pad_token_id=None, output_hidden_states=False, return_dict_in_generate=False, use_cache=None,
                 keep_last_step_only=False, kv_cache_dtype=None, sampler=None, ngram_ban=None, length_penalty=1.0, early_stopping=False,
                 num_return_sequences=1, prompt_lookup_num_tokens=None, max_matching_ngram_size=None, output_logprobs=False, **kwargs):
        """Token-by-token decoding with HF GenerationMixin's greedy / sampling semantics (the reference inherits `generate`):
        every step goes through `prepare_inputs_for_generation` (position_ids = cumsum(attention_mask) - 1, so left-padded batches
        get the reference's RoPE positions); `eos_token_id` defaults to `config.eos_token_id` (int or list); rows that have emitted
        EOS are tracked per row, keep receiving `pad_token_id` (default: the EOS id, as HF does for open-ended generation) and the
        loop ends when every row is finished or a stopping criterion fires.
        use_cache=False reproduces the reference checkpoints' behaviour (config.use_cache=False: every step re-runs the multimodal
        prefill); use_cache=True prefills once and then streams the weights once per token through the GEMV kernels
        with a KV cache.  Greedy (`do_sample=False`) is deterministic; sampling draws from torch's RNG on
        softmax(logits / temperature) with optional nucleus filtering.
        kv_cache_dtype="fp8_e4m3" (bf16 models, use_cache=True) keeps the KV cache as e4m3 codes with per-position scales (KVCache);
        the result equals the same run with a bf16 cache holding the dequantized positions, bit for bit.
        sampler="device" (opt-in; None and "host" are the torch path above) draws each sampled token in one launch (ops.sample_step: the
        same distribution, the same torch noise, so a seeded run draws the host path's tokens) inside the device-resident loop greedy
        decoding uses.  That loop looks at the host every 8 steps, so it may run up to 7 steps past the point where every row had
        finished: the returned ids are trimmed and equal, but the global generator has advanced further than on the host path.
        It does not combine with `no_repeat_ngram_size` (host-side list work) unless ngram_ban="device".
        ngram_ban="device" (opt-in, needs no_repeat_ngram_size >= 1; None and "host" are the list rule on the host, which sends every
        decoding to the per-step host loop): the ban is one launch per step (ops.ngram_ban: a copy of the last-position logits with -inf
        at the tokens `no_repeat_ngram_banned_tokens` names, read from the ids on the device).  Greedy decoding and sampler="device" then
        stay in the device-resident loop and pick from that copy; the host sampler keeps its loop and only skips the tolist() and the
        Python rule.  The ids are the host ban's, bit for bit, from the same logits; `logprobs` still score the raw logits.  GPU tensors
        only.  Prompt-lookup stays refused with either ban: a draft is the continuation of a repeated n-gram, what the ban forbids.
        prompt_lookup_num_tokens=k (opt-in, 1..15; HF's option of the same name, with max_matching_ngram_size, default 2): prompt-lookup
        speculative decoding.  Each step drafts up to k tokens by copying what followed an earlier occurrence of the row's trailing n-gram
        (`prompt_lookup_candidates`), runs ONE forward over the last token and the drafts, and emits the accepted drafts plus one more token
        (ops.spec_step; the cache gives the rejected positions back, KVCache.truncate).  Every emitted token is the token the usual rule --
        argmax, or sampler="device"'s draw on that position's own noise row -- picks from the logits at its position; drafts only decide
        how many positions a forward covers.  The logits of a multi-token forward may differ from a one-token forward's in the last bits, so
        where two candidates are almost tied the ids can differ from the plain loop's.  Batch 1, use_cache=True, no padding, no
        `no_repeat_ngram_size`; sampling needs sampler="device".  The host reads a three-int record every step.  Stopping criteria are
        called once per step on the valid ids, so a criterion can fire up to k tokens later than in the plain loop (HF's assisted decoding
        behaves the same way).
        output_logprobs=True (opt-in; needs return_dict_in_generate=True, a ValueError otherwise, as HF asks for scores): the result carries
        `logprobs`, fp32 [B, n_new] with n_new = sequences.shape[1] - input_ids.shape[1].  Entry [b, j] is the log-probability of the emitted
        token sequences[b, L0 + j] under softmax of the RAW last-position logits of the step that produced it: before temperature, top-k,
        top-p and the n-gram ban, so it says how likely the model itself held the token, whatever the sampling settings (HF's
        `output_logits`, not `output_scores`).  A row that had finished before the step holds a pad-fill token there and gets exactly 0.0;
        a row's EOS token itself gets its real log-probability.  One launch per step (ops.token_logprobs) in every loop; GPU tensors only.
        num_beams=K (2..16; HF's option, with HF's length_penalty=1.0, early_stopping=False / True / "never" and num_return_sequences=1..K):
        deterministic beam search, HF `_beam_search` with do_sample=False -- `generation.beam_search_reference` is the rule, with ties
        between equal scores going to the lowest (beam, token), which HF leaves open.  The state lives on the device (`beam_loop`): per
        step the forward over the B * K running rows, ops.beam_step (two launches) and, with use_cache=True, a reorder of the generated
        positions of the KV cache by the step's parents (KVCache.gather_rows; the prompt's K / V is equal in an item's beams and stays).
        The prefill runs once per item, not once per beam.  Returns the best num_return_sequences finished hypotheses per item, [B * n, L]
        with pad fill behind each row's end; with return_dict_in_generate=True the result also carries `sequences_scores`, fp32 [B * n]
        (the sum of log-probabilities divided by length ** length_penalty).  The host reads one word per step every 8 steps, so up to 7
        forwards may run past the stop; they change nothing.  GPU tensors only.  Not with: sampling, sampler="device", prompt lookup,
        stopping_criteria, output_hidden_states (so not through evaluate()), output_logprobs, kv_cache_dtype, or `no_repeat_ngram_size`
        without ngram_ban="device".  num_beams=1 is the decoding above, unchanged, and refuses the three beam options.
        past_key_values (opt-in, default None; taken by keyword from **kwargs, the one keyword read there -- `output_logprobs` stays the last
        named parameter, which callers and tests rely on -- and every other unknown keyword keeps raising TypeError; a KVCache -- `new_kv_cache()` makes an empty one -- or an HF legacy tuple / Cache object, converted by
        KVCache.from_hf): continue an earlier call's KV cache, with HF's semantics: `input_ids` [B, L] is the WHOLE conversation so far and
        the cache covers its first `cache.length` positions.  It implies use_cache=True.  A KVCache remembers the ids it was filled with
        (`cache.ids`): one launch (ops.ids_common_prefix) compares them with `input_ids` and the cache is cut to the prefix all rows share
        (an edited last turn, another question about the same image), and to L - 1 at most, so that at least one token is fed (HF's rule);
        the ids of an HF cache are unknown and the caller is trusted.  ONLY THE IDS ARE COMPARED, NOT THE IMAGES: a caller who changes the
        image under equal ids gets the old image's keys, as in HF.  Step 0 then feeds the ids behind the kept positions in one forward
        (`images` / `videos` are ignored for a non-empty cache, as the later steps ignore them; placeholder ids among the ids to feed raise
        NotImplementedError).  `attention_mask` is [B, L] over the whole conversation; in the cached columns it may differ from the mask the
        cache was filled under only by clearing the pad fill behind a row's last visible cached position (ValueError otherwise), so every
        visible key keeps the RoPE position a one-shot run gives it.  The cache is advanced IN PLACE (and grown in place when it is too
        small, KVCache.grow): after the call it covers every position that was fed, sequences.shape[1] - 1 of them.  An EMPTY KVCache is
        filled by the call: how a first turn obtains a cache to keep.  With return_dict_in_generate=True the result carries
        `past_key_values` (the same object), and `hidden_states` holds the last-layer states of ALL positions, the earlier calls' included.
        Every loop but beam search, both cache dtypes (the cache's own decides; a contradicting `kv_cache_dtype` is refused).
        `KVCache.fork()` gives an independent copy for several continuations of one prefix.
        stop_strings / tokenizer (opt-in, default None; HF's names, taken by keyword from **kwargs like `past_key_values`): a str or a list
        of str on which a ROW stops, decided on the device -- what the reference's callers ask of KeywordsStoppingCriteria, without the host
        read and the decode of all generated tokens per step, and for every row of a batch, not row 0 alone.  `tokenizer` is required with
        it (ValueError otherwise, as in HF); empty strings and strings holding U+FFFD are refused; at most ops.STOP_MAX_STRINGS strings of
        ops.STOP_MAX_BYTES UTF-8 bytes each.  The rule is `generation.stop_strings_reference`: the row's text is the concatenation of the
        bytes its GENERATED ids stand for (`generation.token_byte_table`: a piece's UTF-8 in context, the raw byte of a byte-fallback token,
        nothing for special ids and for ids the tokenizer does not know), and the row stops after the first generated token inside whose
        bytes a stop string ends.  That token is kept and its log-probability with it, as an EOS token's; the prompt never counts, nor does
        the text of earlier turns under `past_key_values` (L0 is this call's input_ids.shape[1]).  One more launch per step
        (ops.stop_strings) behind the pick in the device-resident loop -- greedy and sampler="device", with or without ngram_ban="device",
        output_logprobs, kv_cache_dtype -- which keeps looking at the host every 8 steps; the host sampler's loop calls the same kernel on its
        ids.  A stopped row is pad-filled from the next step on (a batch needs a pad or EOS id for that), and ids, cache, hidden states and
        log-probabilities are trimmed to the last row's stop as they are for EOS.  The stop string is not cut from the result.  The
        tokenizer's table is built on first use and kept on the model under the tokenizer's identity (rebuilt when len(tokenizer) or the
        vocabulary size changes).  `stopping_criteria` may be passed beside it and forces the per-step host check as before.  GPU tensors
        only; refused with num_beams > 1 and with prompt_lookup_num_tokens.  Differences from tools.KeywordsStoppingCriteria: that criterion
        never checks after the FIRST generated token (a string wholly inside it stops one token earlier here); decode() strips one leading
        space of the whole text (equal positions are claimed for stop strings that do not begin with a space); and its decoder turns a whole
        run of byte tokens into U+FFFD when the run is not valid UTF-8 as it stands, where this rule reads each byte."""
        cfg = self.config
        past_key_values = kwargs.pop("past_key_values", None)
        stop_strings, tokenizer = kwargs.pop("stop_strings", None), kwargs.pop("tokenizer", None)
        eos = cfg.eos_token_id if eos_token_id is None else eos_token_id
        eos_list = [] if eos is None else [eos] if isinstance(eos, int) else list(eos)
        ngram, sampling, device_sampler, use_cache, lookup = check_generate_args(
            input_ids, attention_mask, do_sample=do_sample, temperature=temperature, num_beams=num_beams, no_repeat_ngram_size=no_repeat_ngram_size,
            use_cache=use_cache, kv_cache_dtype=kv_cache_dtype, sampler=sampler, prompt_lookup_num_tokens=prompt_lookup_num_tokens,
            max_matching_ngram_size=max_matching_ngram_size, output_logprobs=output_logprobs, return_dict_in_generate=return_dict_in_generate,
            unknown=kwargs, dtype=self.dtype, vocab_size=cfg.vocab_size, config_use_cache=cfg.use_cache, ngram_ban=ngram_ban,
            length_penalty=length_penalty, early_stopping=early_stopping, num_return_sequences=num_return_sequences,
            stopping_criteria=stopping_criteria, output_hidden_states=output_hidden_states, n_eos=len(eos_list), past_key_values=past_key_values,
            cache_shape=(cfg.num_hidden_layers, cfg.num_attention_heads, cfg.hidden_size // cfg.num_attention_heads), stop_strings=stop_strings,
            tokenizer=tokenizer)
        device_ban = check_ngram_ban(ngram_ban)
        stops = check_stop_strings(stop_strings, tokenizer)
        seq = input_ids
        eos_ids = None if eos is None else torch.as_tensor(eos_list, device=seq.device, dtype=seq.dtype)
        pad = pad_token_id if pad_token_id is not None else getattr(cfg, "pad_token_id", None)
        if pad is None and eos_ids is not None:
            pad = int(eos_ids[0])
        # No padding anywhere (no mask given, or a mask of ones -- one host read, here): the steps run without a key mask.  The results
        # are the same (position_ids = cumsum(ones) - 1 = arange; every key attended) and the attention kernels skip their per-key
        # mask loads, which sit on the latency chain of every decode step.
        no_pad = attention_mask is None or bool(attention_mask.ne(0).all())
        crit = [] if stopping_criteria is None else (list(stopping_criteria) if isinstance(stopping_criteria, (list, tuple)) else [stopping_criteria])
        cache = None
        if use_cache:
            # the prefill fills it; room for every token fed (the last one emitted never is), and for a verify step's drafts
            H, room = cfg.num_attention_heads, max_new_tokens + 1 + (lookup[0] if lookup is not None else 0)
            if past_key_values is None:
                cache = KVCache(cfg.num_hidden_layers, seq.shape[0], H, cfg.hidden_size // H, max(seq.shape[1] + room, 64), seq.device, self.dtype,
                                kv_dtype=kv_cache_dtype)
                cache._id_chunks, cache.borrow_ids = None, True  # the call's own cache goes with the call: no ids remembered, no mask copied
            else:
                cache = past_key_values
                if not isinstance(cache, KVCache):
                    cache = KVCache.from_hf(cache, headroom=room, kv_dtype=kv_cache_dtype)
                enter_cache(cache, seq, attention_mask, no_pad, seq.shape[1] + room, None if self.mm_token_ids is None else self.mm_token_ids.values())
        d = Decoding(self, images, videos, attention_mask, no_pad, cache, max_new_tokens, sampling, temperature, top_k, top_p, eos_ids, pad, crit,
                     output_hidden_states, keep_last_step_only, output_logprobs)
        d.return_cache = past_key_values is not None
        if stops is not None:
            if pad is None and seq.shape[0] > 1:
                raise ValueError("`stop_strings` on a batch needs a `pad_token_id` (or an `eos_token_id`): a row that has stopped is filled with it "
                                 "while the others go on")
            d.stops = (stop_table(self, tokenizer, seq.device), ops.StopStrings(stops, seq.device))
        if num_beams > 1:
            seq, scores = beam_loop(d, seq, num_beams, ngram, length_penalty, early_stopping, num_return_sequences)
            return GenerateOutput(sequences=seq, hidden_states=None, sequences_scores=scores) if return_dict_in_generate else seq
        if d.return_cache:
            # inside this call the cache notes the loops' id tensors as they come, without a copy per step: they are the loops' own buffers
            # and are joined into a tensor of the cache's own before the call returns or raises
            cache.borrow_ids = True
        try:
            if lookup is not None:
                seq, logprobs = prompt_lookup_loop(d, seq, lookup)
            elif (not sampling or device_sampler) and (ngram == 0 or device_ban) and seq.is_cuda:
                seq, logprobs = fused_loop(d, seq, ngram)
            else:
                seq, logprobs = host_loop(d, seq, ngram, sampling_probs, device_ban)
        finally:
            if d.return_cache:
                cache.borrow_ids = False
                cache.own_ids()
        return d.result(seq, logprobs, return_dict_in_generate)
