"""UllavaForCausalLM on MI355X: u-LLaVA core + [SEG]/[LOC] projectors + SAM prompt-encoder / mask-decoder / postprocess.

Host-side mirror of reference `models/ullava.py:69-434` (same constructor, attribute names `.llm .seg_projector
.visual_model .det_projector .det_decoder`, state-dict keys, `forward(..., inference=True)` dict keys and `evaluate()`
tuple).  Differences that are deliberate and output-preserving:
  * the [SEG]/[LOC] rows are gathered BEFORE the projector MLPs (the reference projects all B*S rows and then masks);
  * the SAM image encoder runs batched instead of one image per python iteration with empty_cache();
  * the dense positional encoding is evaluated once (the reference recomputes it per image).
"""
from typing import List, Optional

import torch
import torch.nn as nn

from . import autograd_ops as A
from . import ops
from .configuration import UllavaConfig
from .generation import check_generate_args
from .kv_cache import KVCache
from .modeling_core import BF16, Linear, UllavaCoreForCausalLM, _Holder
from .sam import SamEngine, build_sam_holder



def _mlp_seq(dims, device, dtype, dropout_tail=False):
    """nn.Sequential(Linear, ReLU, Linear, ...) with the reference's child indices (ReLU / Dropout hold no parameters)."""
    mods = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        mods.append(Linear(a, b, device=device, dtype=dtype))
        if i < len(dims) - 2:
            mods.append(nn.ReLU(inplace=True))
    if dropout_tail:
        mods.append(nn.Dropout(0.0))
    return nn.Sequential(*mods)


class UllavaForCausalLM(nn.Module):
    config_class = UllavaConfig

    def __init__(self, config: UllavaConfig, device=None, dtype=BF16):
        super().__init__()
        self.config = config
        llm_config = config.llm_config
        self.llm = UllavaCoreForCausalLM(llm_config, device=device, dtype=dtype)
        D, O = llm_config.hidden_size, config.out_dim
        self.seg_projector = _mlp_seq([D, D, O], device, dtype, dropout_tail=True)            # ullava.py:113-118
        self.visual_model = build_sam_holder(config.sam_config, device=device, dtype=dtype)   # ullava.py:124 (build_sam_vit_h)
        self.det_projector = _mlp_seq([D, D, O], device, dtype, dropout_tail=True)            # ullava.py:86-91
        self.det_decoder = _mlp_seq([O, O, O // 2, 4], device, dtype)                         # ullava.py:96-102
        self._sam = SamEngine(self.visual_model, config.sam_config)
        # trainability defaults of the reference's constructor (ullava.py:84-130): the projectors and the box decoder are trainable,
        # SAM is frozen except -- with config.train_mask_decoder -- its mask decoder.  (The language model's parameters default to
        # frozen here; train_ullava.py:239-261 switches on what it trains by name, exactly as it does for the reference.)
        for mod in (self.seg_projector, self.det_projector, self.det_decoder):
            for p_ in mod.parameters():
                p_.requires_grad = True
        if getattr(config, "train_mask_decoder", True):
            for p_ in self.visual_model.mask_decoder.parameters():
                p_.requires_grad = True
        self.overlap_sam_encoder = True     # SAM image encoder on a second HIP stream beside CLIP + LLaMA (False: same stream)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=None, device=None, **kwargs):
        """reference: inference_ullava.py:37, evaluation/eval_ullava.py:135, webui/gradio_chat.py:26."""
        from .checkpoint import ullava_from_pretrained
        return ullava_from_pretrained(cls, pretrained_model_name_or_path, torch_dtype, device, **kwargs)

    @property
    def weight_quantization(self):
        return self.llm.weight_quantization

    @property
    def activation_quantization(self):
        return self.llm.activation_quantization

    @property
    def decode_activation_quantization(self):
        return self.llm.decode_activation_quantization

    def quantize_weights(self, fmt: str = "fp8_e4m3", activations=None, activation_scope: str = "prefill", decode_activations=None):
        """FP8 ("fp8_e4m3") or MXFP4 ("mxfp4") weight-only inference for the language model (UllavaCoreForCausalLM.quantize_weights); SAM and
        the heads keep their dtype.  activations="fp8_e4m3" (fp8 weights only) / "mxfp8_e4m3" / "mxfp4_e2m1" (mxfp4 weights only): fp8 / fp4 activations in the LLaMA
        prefill as well; activation_scope="prefill+decode" (fp8 weights and activations only): also in decode steps of 5 to 32 tokens;
        decode_activations="mxfp8_e4m3" (mxfp4 weights only, with any prefill mode): MXFP8 activations in decode steps of 5 to 32 tokens
        (W4A8 from the resident codes); `decode_activation_quantization` reports it."""
        self.llm.quantize_weights(fmt, activations=activations, activation_scope=activation_scope, decode_activations=decode_activations)
        return self

    @property
    def sam_attention(self) -> str:
        return self._sam.global_attention

    def set_sam_attention(self, mode: str = "exact"):
        """How the SAM image encoder's global blocks (64 x 64 grid, 4096 keys) round their softmax in inference encodes (`forward` without
        gradients through SAM and `evaluate`; the encoder is frozen, the training graph does not contain it and is not affected):
        "streamed" (default) rounds exp(s - running max) and divides by the row sum at the end; "exact" normalises in fp32 and rounds
        afterwards, as the reference does (image_encoder.py:251-253), at about twice the attention time -- the per-op block loop with
        `ops.sam_global_attention_exact`.  A global block without such a kernel then raises NotImplementedError."""
        if mode not in SamEngine.GLOBAL_ATTENTION_MODES:
            raise ValueError(f"sam attention mode must be one of {SamEngine.GLOBAL_ATTENTION_MODES}, got {mode!r}")
        self._sam.global_attention = mode
        return self

    @property
    def sam_precision(self):
        return self._sam.linear_precision

    def set_sam_precision(self, mode="fp8_e4m3"):
        """The number format of the SAM image encoder's Linears in inference encodes (`forward` and `evaluate`; the encoder is frozen and the
        training graph does not contain it).  None (default): the model's bf16 GEMMs, bit-identical to a model never switched.  "fp8_e4m3"
        (bf16 models only; NotImplementedError names any other dtype): qkv, proj, lin1 and lin2 of all ViT blocks run W8A8 -- weights as
        `ops.quantize_fp8` codes with one power-of-two scale per row, input rows quantized per token by the same rule (inside the LayerNorm
        launch where the normed rows feed nothing else), the product on the block-scaled fp8 matrix instruction, bias / GELU / residual at the
        bf16 Linear's rounding points.  Patch and position embedding, attention and rel-pos, the neck, the prompt encoder and the mask decoder
        stay bf16.  The per-op block loop runs (as under set_sam_attention("exact"), with which it combines).  The fp8 codes are derived data
        beside the bf16 parameters -- about 0.63 GB more for ViT-H, built at the first fp8 encode and dropped by a reload or a cast -- so
        state_dict, save_pretrained, training and switching back to None keep working.
        Measured on one MI355X (profiles/sam_fp8.txt, random-init weights, arms interleaved): the 32-block encoder 9.90 -> 8.31 ms at B = 1
        (0.84 x) and 51.4 -> 48.1 ms at B = 8 (0.94 x); one RES step at batch 8 88.2 -> 85.8 ms (0.974 x, just outside the 2 % box spread).
        At B = 8 the fp8 GEMM alone is 0.78-0.92 x the bf16 launch, qkv and lin1 with the fused norm 0.87-0.89 x, but proj and lin2 with their
        row quantization launch are SLOWER than bf16 (1.10 x, 1.12 x).  Encoder output against bf16: mean |d| 1.2e-3, max 2.0e-2 on mean |y|
        1.2e-2; mask logits mean |d| 7.6e-7 on mean 2.9e-5, 99.1 % of the signs equal.  Task accuracy on real checkpoints is not measured."""
        if mode not in SamEngine.LINEAR_PRECISIONS:
            raise ValueError(f"sam precision must be one of {SamEngine.LINEAR_PRECISIONS}, got {mode!r}")
        dtype = self.visual_model.image_encoder.pos_embed.dtype
        if mode is not None and dtype != BF16:
            raise NotImplementedError(f"set_sam_precision({mode!r}) needs a bfloat16 model, this one is {dtype}")
        self._sam.linear_precision = mode
        return self

    def save_pretrained(self, save_directory, **kwargs):
        if self.llm.weight_quantization is not None:
            self.llm._refuse_quantized("save_pretrained")
        from .checkpoint import save_pretrained
        return save_pretrained(self, save_directory, **kwargs)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        sd = {k.replace("llm.vision_encoder.vision_model.", "llm.vision_encoder."): v for k, v in state_dict.items()}
        sd = {k: v for k, v in sd.items() if not k.endswith("position_ids") and "rotary_emb.inv_freq" not in k}
        self.llm._packed = None
        self._sam.invalidate()
        return super().load_state_dict(sd, strict=strict, assign=assign)

    def load_visual_checkpoint(self, checkpoint):
        """reference ullava.py:134-137."""
        with open(checkpoint, "rb") as f:
            sd = torch.load(f, map_location="cpu", weights_only=True)      # a plain tensor state-dict (sam_vit_h_4b8939.pth)
        self._sam.invalidate()
        return self.visual_model.load_state_dict(sd, strict=False)

    @property
    def dtype(self):
        return self.llm.dtype

    @property
    def device(self):
        return self.llm.device

    def _apply(self, fn, *args, **kwargs):
        if self.llm.weight_quantization is not None:
            self.llm._refuse_cast(fn)                       # before any submodule is converted
        out = super()._apply(fn, *args, **kwargs)           # (the core model invalidates its own packs in its _apply)
        self._sam.invalidate()
        self._side = None
        return out

    def _side_stream(self):
        if not self.overlap_sam_encoder:
            return torch.cuda.current_stream()
        st = getattr(self, "_side", None)
        if st is None:
            st = self._side = torch.cuda.Stream()
        return st

    # -- SAM image encoder -------------------------------------------------------------------------------------------
    def _visual_embs_tm(self, pixel_values: torch.Tensor) -> torch.Tensor:
        return self._sam.encode(pixel_values)                       # [B, g*g, 256] token-major

    def get_visual_embs(self, pixel_values: torch.FloatTensor) -> torch.Tensor:
        """reference ullava.py:139-150 -> [B, 256, g, g] (NCHW, as the reference returns it)."""
        tm = self._visual_embs_tm(pixel_values)
        B, P, C = tm.shape
        g = int(P ** 0.5)
        return tm.view(B, g, g, C).permute(0, 3, 1, 2).contiguous()

    # -- shared tail of forward / evaluate -----------------------------------------------------------------------------
    def _heads_training_graph(self) -> bool:
        """gradients enabled and one of the heads on top of the language model is trainable (train_ullava.py:248-261: seg / det
        projectors, det_decoder, mask_decoder)."""
        if not torch.is_grad_enabled() or self.dtype == torch.float32:        # (the fp32 build is inference-only: csrc/f32.hip has no backward)
            return False
        mods = (self.seg_projector, self.det_projector, self.det_decoder, self.visual_model.mask_decoder)
        return any(p.requires_grad for m in mods for p in m.parameters())

    def _run_mlp(self, seq, x, train: bool = False):
        lin = [m for m in seq if isinstance(m, Linear)]
        for i, l in enumerate(lin):
            if train:
                x = A.linear(x, l.weight, l.bias, relu=i < len(lin) - 1)
            else:
                x = ops.linear(x, l.weight, l.bias, act="relu" if i < len(lin) - 1 else None)
        return x

    def _select(self, last_hidden: torch.Tensor, token_mask: torch.Tensor, projector, train: bool = False) -> List[torch.Tensor]:
        """rows of last_hidden [B, L, D] where token_mask [B, L] is set -> per-sample [n_i, out_dim] after the projector."""
        B, L, D = last_hidden.shape
        counts = token_mask.sum(-1).tolist()                       # host sync (the reference indexes device offsets too)
        idx = token_mask.reshape(-1).nonzero().squeeze(-1)
        if train:
            rows = last_hidden.reshape(B * L, D)[idx]               # gather (data movement) recorded by autograd
        else:
            rows = ops.gather_rows(last_hidden.reshape(B * L, D), idx)
        emb = self._run_mlp(projector, rows, train) if rows.shape[0] else rows.new_empty(0, self.config.out_dim)
        out, o = [], 0
        for c in counts:
            out.append(emb[o:o + c])
            o += c
        return out

    def _decode(self, image_embeddings_tm, pred_embeddings, resize_list, size_list, train: bool = False):
        """prompt encoder + mask decoder + postprocess.  The reference decodes one image at a time (ullava.py:228-252); every op of
        the decoder is independent per prompt, so all prompts of the batch go through one chain of launches here (the per-image
        chains were host-launch-bound: ~70 small kernels each) and only the two resizes of postprocess_masks stay per image."""
        counts = [int(e.shape[0]) for e in pred_embeddings]
        dev = image_embeddings_tm.device
        low_all = None
        if sum(counts):
            idx = torch.tensor([i for i, c in enumerate(counts) for _ in range(c)], dtype=torch.int64, device=dev)
            text = torch.cat([e for e in pred_embeddings if e.shape[0]], dim=0).contiguous()
            if train:
                masks = self._sam.decode_train(image_embeddings_tm, text, idx)
            else:
                masks, _iou = self._sam.decode(image_embeddings_tm, text, idx)
            low_all = masks[:, 0].contiguous()                      # multimask_output=False -> mask 0
        pred_masks, o = [], 0
        for i, c in enumerate(counts):
            H, W = int(size_list[i][0]), int(size_list[i][1])
            if c == 0:
                pred_masks.append(torch.empty(0, H, W, device=dev, dtype=torch.float32))
                continue
            post = self._sam.postprocess_train if train else self._sam.postprocess
            pred_masks.append(post(low_all[o:o + c].contiguous(), resize_list[i], (H, W)))
            o += c
        return pred_masks

    def forward(self, images_sam: torch.FloatTensor, images: torch.FloatTensor, input_ids: torch.LongTensor, labels: torch.LongTensor,
                attention_mask: torch.LongTensor, mask_list: List[torch.FloatTensor], size_list: List[torch.Tensor],
                resize_list: List[tuple], bbox_list: List[torch.FloatTensor], inference: bool = False):
        """reference ullava.py:152-333.  inference=False returns the training-loss dict; with gradients enabled and trainable
        parameters (train_ullava.py:207-261) the losses carry an autograd graph whose backward runs HIP kernels (autograd_ops.py)."""
        B = input_ids.shape[0]
        # the SAM image encoder does not depend on the LLM: it runs on a second HIP stream and fills the gaps (tile-quantisation
        # tails, small kernels, launch latency) of the CLIP + LLaMA stream; joined before the mask decoder.  Each stream has its own
        # stream-K workspace (ops._streamk_ws); while both are busy the K-split of partial tile rounds is limited to K >= 8192 because the
        # CUs it would fill are not idle (policy only -- correctness does not depend on it).
        main = torch.cuda.current_stream()
        side = self._side_stream()
        side.wait_stream(main)
        with ops.streamk_policy(8192 if side is not main else 2048):
            with torch.cuda.stream(side), torch.no_grad():          # SAM image encoder: frozen (reference get_visual_embs: no_grad)
                image_embeddings = self._visual_embs_tm(images_sam)
            pad = torch.zeros((B, 1), dtype=torch.bool, device=input_ids.device)
            seg_token_mask = torch.cat([input_ids[:, 1:] == self.config.seg_token_idx, pad], dim=1)    # row t selected iff ids[t+1]==[SEG]
            loc_token_mask = torch.cat([input_ids[:, 1:] == self.config.loc_token_idx, pad], dim=1)
            output = self.llm.forward(images=images, attention_mask=attention_mask, input_ids=input_ids, labels=labels,
                                      output_hidden_states=True)
        last = output.hidden_states[-1]
        main.wait_stream(side)
        image_embeddings.record_stream(main)
        train = self._heads_training_graph() and not inference
        pred_embeddings = self._select(last, seg_token_mask, self.seg_projector, train)
        pred_loc_embeddings = self._select(last, loc_token_mask, self.det_projector, train)
        pred_masks = self._decode(image_embeddings, pred_embeddings, resize_list, size_list, train)
        pred_boxes = [self._run_mlp(self.det_decoder, e, train) if e.shape[0] else e.new_empty(0, 4) for e in pred_loc_embeddings]
        if inference:
            return {"pred_masks": pred_masks, "pred_boxes": pred_boxes, "gt_masks": mask_list, "gt_boxes": bbox_list, "logits": output.logits}
        return self._losses(output.loss, pred_masks, pred_boxes, mask_list, bbox_list, train)

    def _losses(self, ce, pred_masks, pred_boxes, gt_masks, gt_boxes, train: bool = False):
        """reference ullava.py:268-333 + models/loss.py.  The per-pixel / per-box sums are HIP kernels; the handful of scalar
        combinations below run as 0-dim device ops.  Like the reference, the total is accumulated IN PLACE into the tensor that
        `ce_loss` names, so the returned "ce_loss" equals "loss" (reproduced, not corrected)."""
        cfg = self.config
        if ce is None:
            raise ValueError("forward(inference=False) needs `labels` (the reference multiplies output.loss by ce_weight)")
        ce_loss = ce * cfg.ce_weight
        loss = ce_loss
        dev = ce_loss.device
        mask_bce = torch.zeros((), device=dev)
        mask_dice = torch.zeros((), device=dev)
        box_l1 = torch.zeros((), device=dev)
        box_giou = torch.zeros((), device=dev)
        num_masks = num_boxes = 0
        for i in range(len(pred_masks)):
            gm, pm = gt_masks[i], pred_masks[i]
            if gm.shape[0] != pm.shape[0]:
                raise AssertionError(f"gt_mask.shape: {tuple(gm.shape)}, pred_mask.shape: {tuple(pm.shape)}")
            n = gm.shape[0]
            if n:
                sums = (A.mask_loss_sums if train else ops.mask_loss_sums)(pm.contiguous(), gm.to(device=dev, dtype=torch.float32).contiguous())   # [n, 4]
                hw = pm[0].numel()
                mask_bce = mask_bce + (sums[:, 0] / hw).sum() / (n + 1e-8) * n
                dice = 1 - (2 * sums[:, 1] + 1e-6) / (sums[:, 2] + sums[:, 3] + 1e-6)
                mask_dice = mask_dice + dice.sum() / (n + 1e-8) * n
            num_masks += n
            gb, pb = gt_boxes[i], pred_boxes[i]
            if gb.shape[0] != pb.shape[0]:
                raise AssertionError(f"gt_box.shape: {tuple(gb.shape)}, pred_box.shape: {tuple(pb.shape)}")
            nb = gb.shape[0]
            if nb:
                bl = (A.box_losses if train else ops.box_losses)(pb, gb.to(device=dev, dtype=torch.float32))
                box_l1 = box_l1 + bl[0] / (nb + 1e-8)
                box_giou = box_giou + bl[1] / (nb + 1e-8)
            num_boxes += nb
        mask_bce_loss = cfg.bce_weight * mask_bce / (num_masks + 1e-8)
        mask_dice_loss = cfg.dice_weight * mask_dice / (num_masks + 1e-8)
        mask_loss = mask_bce_loss + mask_dice_loss
        box_l1_loss = cfg.l1_weight * box_l1 / (num_boxes + 1e-8)
        box_giou_loss = cfg.iou_weight * box_giou / (num_boxes + 1e-8)
        bbox_loss = box_l1_loss + box_giou_loss
        loss += mask_loss
        loss += bbox_loss
        return {"loss": loss, "ce_loss": ce_loss, "mask_bce_loss": mask_bce_loss, "mask_dice_loss": mask_dice_loss, "mask_loss": mask_loss,
                "bbox_loss": bbox_loss}

    @torch.no_grad()
    def evaluate(self, images_sam, images, input_ids, raw_size_list, resize_list, max_new_tokens=32, temperature=0.2, top_p=None,
                 num_beams=1, no_repeat_ngram_size=None, stopping_criteria=None, kv_cache_dtype=None, stop_strings=None, tokenizer=None,
                 ngram_ban=None, past_key_values=None, prompt_lookup_num_tokens=None, max_matching_ngram_size=None, output_logprobs=False,
                 sampler=None):
        """reference ullava.py:335-434 -> (output_ids, pred_masks, pred_boxes).  kv_cache_dtype="fp8_e4m3": generate with an fp8 KV cache
        (which implies use_cache=True; see UllavaCoreForCausalLM.generate).  sampler="device": draw the tokens with the on-device sampler
        (same ids under the same seed; see generate).  ngram_ban="device" (with no_repeat_ngram_size): the n-gram ban in one launch per step, so
        that greedy decoding and sampler="device" keep the device-resident loop (the host ban's ids; see generate).
        prompt_lookup_num_tokens / max_matching_ngram_size: prompt-lookup speculative decoding
        (which implies use_cache=True; batch 1; with temperature > 0 it needs sampler="device"; see generate) -- the [SEG] / [LOC] rows are
        read from the hidden states of the accepted positions.  output_logprobs=True: the return grows to (output_ids, pred_masks, pred_boxes,
        logprobs), logprobs fp32 [B, n_new] as generate(output_logprobs=True) gives them (raw distribution; 0.0 after a row's EOS) -- the
        number to drop an unsure [SEG] / [LOC] by.
        past_key_values (a KVCache; `new_kv_cache()` makes an empty one for the first turn): continue an earlier call's cache, as
        generate(past_key_values=) does (which implies use_cache=True; `input_ids` is the whole conversation; only the ids are compared with
        what the cache holds, NOT the images -- a changed image under equal ids gets the old image's keys, as in HF).  The cache is advanced
        in place and also keeps the SAM image embeddings of the call that computed them (`cache.side["sam_image_embeddings"]`, keyed to
        nothing else): while they are there the SAM encoder does not run.  Masks and boxes are computed from the hidden states of all
        positions, the earlier calls' included: what the reference yields when it is fed the whole conversation.
        stop_strings / tokenizer: stop each row on text, decided on the device (HF's names; what the reference's scripts ask of
        KeywordsStoppingCriteria([stop_str], tokenizer, input_ids) -- see generate for the rule and its documented differences)."""
        # generate()'s refusals, before the SAM encoder starts (the model's dtype is asked for only where kv_cache_dtype needs it)
        gen = dict(do_sample=temperature > 0, temperature=temperature, num_beams=num_beams, no_repeat_ngram_size=no_repeat_ngram_size,
                   sampler=sampler, return_dict_in_generate=True, output_logprobs=output_logprobs, kv_cache_dtype=kv_cache_dtype,
                   prompt_lookup_num_tokens=prompt_lookup_num_tokens, max_matching_ngram_size=max_matching_ngram_size, ngram_ban=ngram_ban,
                   use_cache=True if kv_cache_dtype is not None or prompt_lookup_num_tokens is not None or past_key_values is not None else None)
        gen_shape = None
        if stop_strings is not None or tokenizer is not None:
            gen["stop_strings"], gen["tokenizer"] = stop_strings, tokenizer
        if past_key_values is not None:
            gen["past_key_values"] = past_key_values                # (a call without one hands generate() exactly the keywords it always did)
            lc = self.llm.config                                    # (the model's geometry is asked for only where a cache is held against it)
            gen_shape = (lc.num_hidden_layers, lc.num_attention_heads, lc.hidden_size // lc.num_attention_heads)
        check_generate_args(input_ids, dtype=None if kv_cache_dtype is None else self.llm.dtype, output_hidden_states=True,
                            cache_shape=gen_shape, **gen)
        kept = past_key_values.side if isinstance(past_key_values, KVCache) else None
        image_embeddings = None if kept is None else kept.get("sam_image_embeddings")
        main = side = torch.cuda.current_stream()
        if image_embeddings is None:
            side = self._side_stream()                              # SAM image encoder on the second stream, under the generation loop
            side.wait_stream(main)
            with torch.cuda.stream(side):
                image_embeddings = self._visual_embs_tm(images_sam)     # its GEMMs use the side stream's own stream-K workspace
        outputs = self.llm.generate(input_ids=input_ids, images=images, max_new_tokens=max_new_tokens, top_p=top_p, output_hidden_states=True,
                                    stopping_criteria=stopping_criteria, keep_last_step_only=True, **gen)
        output_ids = outputs.sequences
        last = outputs.hidden_states[-1][-1]                          # last step, last layer: [B, L-1, D]
        seg_token_mask = output_ids[:, 1:] == self.config.seg_token_idx
        loc_token_mask = output_ids[:, 1:] == self.config.loc_token_idx
        L1 = last.shape[1]
        pred_embeddings = self._select(last, seg_token_mask[:, :L1], self.seg_projector)
        pred_loc_embeddings = self._select(last, loc_token_mask[:, :L1], self.det_projector)
        if side is not main:
            main.wait_stream(side)
            image_embeddings.record_stream(main)
        if kept is not None:
            # kept only now, behind the wait: a later call reads them on the main stream, ordered after the encoder; a call that raised
            # before this line has kept nothing
            kept["sam_image_embeddings"] = image_embeddings
        pred_masks = self._decode(image_embeddings, pred_embeddings, resize_list, raw_size_list)
        pred_boxes = [self._run_mlp(self.det_decoder, e) if e.shape[0] else e.new_empty(0, 4) for e in pred_loc_embeddings]
        if output_logprobs:
            return output_ids, pred_masks, pred_boxes, outputs.logprobs
        return output_ids, pred_masks, pred_boxes

    def new_kv_cache(self, batch_size: int, capacity: int, kv_cache_dtype=None):
        """UllavaCoreForCausalLM.new_kv_cache of the language model: an empty KVCache for evaluate(past_key_values=) to fill."""
        return self.llm.new_kv_cache(batch_size, capacity, kv_cache_dtype)

    def score(self, input_ids, attention_mask=None, images=None, videos=None, labels=None):
        """UllavaCoreForCausalLM.score of the language model (see there)."""
        return self.llm.score(input_ids, attention_mask=attention_mask, images=images, videos=videos, labels=labels)
