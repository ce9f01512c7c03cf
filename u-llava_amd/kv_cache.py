"""The KV cache of KV-cached LLaMA decoding: per-layer K and V^T in the attention kernels' layouts, in the model dtype or as fp8 (e4m3)
codes with per-position scales, the HF views of it, and the two steps of a decode layer over an fp8 cache."""
import torch

from . import ops

BF16 = torch.bfloat16

KV_CACHE_DTYPES = ("fp8_e4m3",)

# positions past the ones it is handed that a cache gets when forward() has to size it on its own (use_cache=True without a cache, an HF
# tuple as past_key_values): room for a caller-driven decode loop.  generate() sizes its cache from max_new_tokens.
DEFAULT_HEADROOM = 512


def _check_kv_dtype(kv_dtype, dtype):
    """the cache formats there are: None (the model dtype) or "fp8_e4m3" (bf16 models only)."""
    if kv_dtype is None:
        return
    if not isinstance(kv_dtype, str) or kv_dtype not in KV_CACHE_DTYPES:
        raise ValueError(f"unknown KV cache dtype {kv_dtype!r} (supported: None, {', '.join(repr(d) for d in KV_CACHE_DTYPES)})")
    if dtype != BF16:
        raise NotImplementedError(f"an fp8 KV cache needs a bf16 model, not {dtype}: the dequantized values of a position with a small amax "
                                  "can fall below the fp16 range, and the fp32 build has no fp8 kernels")


class KVCache:
    """Per-layer K [B,H,Smax,hd] (post-RoPE) and V^T [B,H,hd,Smax] in the attention kernel's key-permuted layout, plus the
    last-layer hidden states of every position seen so far (what `evaluate()` reads for [SEG]/[LOC] rows).  Truthy once a
    prefill has been stored, like a non-empty HF past_key_values tuple."""

    kv_dtype = None                        # "fp8_e4m3": see below
    _id_chunks = None                      # (a cache made without __init__: ids unknown, no mask recorded)
    mask = None
    borrow_ids = False                     # generate() sets it for the length of a call: see note_fed

    def __init__(self, n_layers, B, H, hd, smax, device, dtype=BF16, kv_dtype=None):
        """kv_dtype="fp8_e4m3" (bf16 models only): the cache holds e4m3fn codes in the same two layouts (k8 [B,H,Smax,hd], vt8 [B,H,hd,Smax])
        plus one fp32 power-of-two scale per (batch, head, position) for the K row (k_scale, by key) and the V column (vt_scale, by V^T slot),
        with the fp8-weight rule (DESIGN f2).  Attention reads the K / V of its own forward call at full bf16 precision and the earlier
        positions dequantized; the new positions are quantized into the cache.  So the model equals, bit for bit, the same model with a bf16
        cache holding the dequantized positions (`dequantized()`).  A decode step's new keys pass through a bf16 staging window (k_stage /
        vt_stage: 128 positions, one window shared by all layers) on their way into the cache."""
        _check_kv_dtype(kv_dtype, dtype)
        self.smax = ((smax + 63) // 64) * 64
        self.length = 0
        self.last_hidden = []
        self._geom = (n_layers, B, H, hd, torch.device(device), dtype)
        self._id_chunks = []               # the ids the positions were filled with (see `ids`); None: unknown
        self.mask = None                   # the attention mask the positions were filled under ([B, length]); None: all ones
        self.side = {}                     # what a caller keeps beside the keys (evaluate(): the SAM image embeddings)
        if kv_dtype is None:
            self.k = [torch.empty(B, H, self.smax, hd, device=device, dtype=dtype) for _ in range(n_layers)]
            self.vt = [torch.zeros(B, H, hd, self.smax, device=device, dtype=dtype) for _ in range(n_layers)]
            return
        self.kv_dtype = kv_dtype
        self.k = self.vt = None
        u8, f32 = torch.uint8, torch.float32
        self.k8 = [torch.zeros(B, H, self.smax, hd, device=device, dtype=u8) for _ in range(n_layers)]
        self.vt8 = [torch.zeros(B, H, hd, self.smax, device=device, dtype=u8) for _ in range(n_layers)]
        self.k_scale = [torch.zeros(B, H, self.smax, device=device, dtype=f32) for _ in range(n_layers)]
        self.vt_scale = [torch.zeros(B, H, self.smax, device=device, dtype=f32) for _ in range(n_layers)]
        self.k_stage = torch.zeros(B, H, 128, hd, device=device, dtype=dtype)
        self.vt_stage = torch.zeros(B, H, hd, 128, device=device, dtype=dtype)
        self._kv8_ptrs = None              # (data_ptr key, ctypes arrays) of c_ptrs()

    def kv8_layer(self, li):
        """(k8, vt8, k_scale, vt_scale) of layer li of an fp8 cache."""
        return self.k8[li], self.vt8[li], self.k_scale[li], self.vt_scale[li]

    def bf16_scratch(self):
        """(fp8 cache) a bf16 K [B,H,Smax,hd] / V^T [B,H,hd,Smax] pair (V^T zero-filled) for the calls the fp8 decode attention does not take
        (<= 64 keys, > 16 new tokens): each layer is dequantized into it, runs the bf16 path, and its new positions are quantized back.
        Made per forward call and shared by its layers; the cache itself keeps no bf16 buffer but the staging window."""
        B, H, smax, hd = self.k8[0].shape
        dev = self.k8[0].device
        return torch.empty(B, H, smax, hd, device=dev, dtype=BF16), torch.zeros(B, H, hd, smax, device=dev, dtype=BF16)

    def _kv8_decode_buffers(self, li: int, past: int, fewq: bool, scr: list):
        """(K, V^T, pitch, position of the first new key) the decode appenders of layer li write into, on an fp8 cache: the staging window
        (first new key at past mod 64) where the fp8 decode attention takes the call (fewq), else the call's bf16 scratch (scr, made on first
        use) with positions < past dequantized."""
        if fewq:
            return self.k_stage, self.vt_stage, 128, past & 63
        if not scr:
            scr.append(self.bf16_scratch())
        kc, vtc = scr[0]
        ops.dequantize_kv(*self.kv8_layer(li), past, k_out=kc, vt_out=vtc)
        return kc, vtc, self.smax, past

    def _kv8_attention(self, q, q_strides, li: int, att, B: int, H: int, S: int, past: int, hd: int, key_mask, fewq: bool, scr: list):
        """the decode attention of layer li over an fp8 cache, after _kv8_decode_buffers' appenders; the new positions end in the cache."""
        if fewq:
            ops.attention_kv8(q, q_strides, self.k_stage, self.vt_stage, *self.kv8_layer(li), att, (S * H * hd, hd, H * hd), B, H, S, past + S,
                              hd, key_mask, hd ** -0.5)
            return
        kc, vtc = scr[0]
        smax = self.smax
        ops.attention(q, kc, vtc, att, B, H, S, past + S, hd, q_strides, (H * smax * hd, smax * hd, hd), (S * H * hd, hd, H * hd), key_mask,
                      causal=True, scale_mode=1, scale=hd ** -0.5)
        ops.quantize_kv(kc, (H * smax * hd, smax * hd, hd), vtc, (H * hd * smax, hd * smax, smax), *self.kv8_layer(li), past, S, src_p0=past,
                        v_image=True)

    def nbytes(self) -> int:
        """bytes of every device buffer the cache keeps (fp8: codes, scales and the staging window; bf16: K and V^T)."""
        ts = (self.k + self.vt) if self.kv_dtype is None else (self.k8 + self.vt8 + self.k_scale + self.vt_scale + [self.k_stage, self.vt_stage])
        return sum(t.numel() * t.element_size() for t in ts)

    def dequantized(self) -> "KVCache":
        """The bf16 twin of an fp8 cache: a bf16 KVCache whose positions < length hold dequant(codes) = float(code) * 2^s (same length,
        same last_hidden).  A bf16 cache returns itself."""
        if self.kv_dtype is None:
            return self
        B, H, smax, hd = self.k8[0].shape
        c = KVCache(len(self), B, H, hd, smax, self.k8[0].device, BF16)
        if self.length:
            for li in range(len(self)):
                ops.dequantize_kv(*self.kv8_layer(li), self.length, k_out=c.k[li], vt_out=c.vt[li])
        c.length = self.length
        c.last_hidden = list(self.last_hidden)
        c._id_chunks, c.mask = self._ids_carried(), self.mask
        return c

    def __bool__(self):
        return self.length > 0

    @property
    def ids(self):
        """int64 [B, length] on the device: the ids the cache was filled with, which forward() appends to when it is handed `input_ids`
        (placeholder ids of image / video patches included); None once a position was fed as `inputs_embeds` or came from `from_hf`.
        The calls' id tensors are kept as they come and joined -- into a tensor of the cache's own -- when this is read."""
        if self._id_chunks is None or sum(c.shape[1] for c, _ in self._id_chunks) != self.length:
            return None                                           # (positions that did not come through forward(): a replicated cache)
        if len(self._id_chunks) != 1 or not self._id_chunks[0][1]:
            B, dev = self._geom[1], self._geom[4]
            ids = torch.cat([c for c, _ in self._id_chunks], dim=1) if self._id_chunks else torch.empty(B, 0, dtype=torch.int64, device=dev)
            self._id_chunks = [(ids, True)]                       # (True: the cache's own copy, no view of a caller's tensor)
        return self._id_chunks[0][0]

    def _ids_carried(self):
        """`_id_chunks` of a copy of this cache (the joined tensor is never written in place: shared)."""
        ids = self.ids
        return None if ids is None else [(ids, True)]

    def own_ids(self) -> None:
        """join what was noted into tensors of the cache's own (ids and mask): no view of a caller's tensor is left behind."""
        self.ids
        if self.mask is not None and not getattr(self, "_mask_own", False):
            self.mask, self._mask_own = self.mask.clone(), True

    def note_fed(self, input_ids, n: int, attention_mask=None) -> None:
        """forward()'s bookkeeping after it has stored n new positions: their ids (None: fed as embeddings, the ids become unknown) and the
        mask the cache now stands under ([B, length] or None).  The cache keeps COPIES: a caller may reuse or overwrite its id buffer and
        its mask after the call (a one-token step copies 8 bytes per row; every 32 calls the copies are joined).  Only inside generate()
        (`borrow_ids`), whose loops own their buffers and which joins them into the cache's own tensor before it returns, the tensors are
        noted as they come, so that a decode step launches nothing for it."""
        own = not self.borrow_ids
        if input_ids is None or tuple(input_ids.shape) != (self._geom[1], n) or input_ids.dtype != torch.int64:
            self._id_chunks = None
        elif self._id_chunks is not None:
            self._id_chunks.append((input_ids.clone() if own else input_ids, own))
            if own and len(self._id_chunks) >= 32:
                self.ids
        self._mask_own = own or attention_mask is None
        if attention_mask is not None and attention_mask.shape[-1] == self.length:
            self.mask = attention_mask.clone() if own else attention_mask
        elif attention_mask is None and self.mask is not None:
            self.mask = torch.cat([self.mask, self.mask.new_ones(self.mask.shape[0], self.length - self.mask.shape[1])], dim=1)
        elif attention_mask is not None:
            self.mask = None                                      # (a mask of another width: what the cache stands under is not known)

    def truncate(self, n: int) -> None:
        """Give back the positions >= n (speculative decoding: the rejected drafts of a verify step): `length` becomes n, `last_hidden`
        holds exactly the first n positions (the last call's tensor is sliced) and so do `ids` and the recorded mask.  bf16 and fp8 caches alike: the buffers keep the rejected
        positions' K rows, V^T columns, codes and scales as stale finite data, which no kernel reads -- attention, append and quantization
        address keys below `length` plus the call's own new positions, and the next call overwrites them."""
        n = int(n)
        if n < 0 or n > self.length:
            raise ValueError(f"KVCache.truncate({n}): the cache holds {self.length} positions")
        self.length = n
        have = sum(h.shape[1] for h in self.last_hidden)
        while self.last_hidden and have > n:
            last = self.last_hidden[-1]
            if have - last.shape[1] >= n:
                self.last_hidden.pop()
                have -= last.shape[1]
            else:
                self.last_hidden[-1] = last[:, :last.shape[1] - (have - n)]
                have = n
        if self._id_chunks is not None:
            have = sum(c.shape[1] for c, _ in self._id_chunks)
            while self._id_chunks and have > n:
                c, own = self._id_chunks[-1]
                if have - c.shape[1] >= n:
                    self._id_chunks.pop()
                    have -= c.shape[1]
                else:
                    self._id_chunks[-1] = (c[:, :c.shape[1] - (have - n)], own)
                    have = n
        if self.mask is not None:
            self.mask = self.mask[:, :n] if n else None
        if n == 0:
            self._id_chunks = []                                   # an empty cache knows its ids again

    def c_ptrs(self):
        """(void* array of the K buffers, void* array of the V^T buffers) for the coarse decode entry; built once per cache.
        fp8 cache: (k8, vt8, k_scale, vt_scale void* arrays, k_stage, vt_stage) for the *_kv8 entries, rebuilt whenever a list entry has
        been rebound since (the arrays hold raw pointers)."""
        if self.kv_dtype is not None:
            import ctypes
            lists = (self.k8, self.vt8, self.k_scale, self.vt_scale)
            key = tuple(t.data_ptr() for l in lists for t in l)
            if self._kv8_ptrs is None or self._kv8_ptrs[0] != key:
                arrs = tuple((ctypes.c_void_p * len(l))(*[t.data_ptr() for t in l]) for l in lists)
                self._kv8_ptrs = (key, arrs + (self.k_stage, self.vt_stage))
            return self._kv8_ptrs[1]
        if getattr(self, "_c_ptrs", None) is None:
            import ctypes
            self._c_ptrs = ((ctypes.c_void_p * len(self.k))(*[t.data_ptr() for t in self.k]), (ctypes.c_void_p * len(self.vt))(*[t.data_ptr() for t in self.vt]))
        return self._c_ptrs

    def _shape(self):
        return tuple(self.k[0].shape) + (self.k[0].element_size(),)     # B, H, smax, hd, bytes per element

    def _copy_into(self, c: "KVCache") -> None:
        """positions < length of every layer into the (fresh, zero-filled where a fresh cache is) buffers of c: the model-dtype caches
        through ops.kv_gather_rows with the identity row map, the fp8 cache through ops.kv8_copy_positions.  gather_rows moves V^T in whole
        32-key blocks, so the slots of the keys length .. of the last block are zeroed again afterwards (a truncated cache holds stale
        values there): beyond the sequence the V^T columns of c are zero, as a fresh cache has them."""
        n = self.length
        if n == 0:
            return
        if self.kv_dtype is not None:
            ops.kv8_copy_positions((self.k8, self.vt8, self.k_scale, self.vt_scale), (c.k8, c.vt8, c.k_scale, c.vt_scale), n)
            return
        B, H, smax, hd, esz = self._shape()
        ops.kv_gather_rows(*self.c_ptrs(), *c.c_ptrs(), len(self.k), B, B, H, hd, esz, smax, c.smax, 0, 0, n, None, None)
        if n & 31:
            slots = torch.tensor([self.vt_slot(p) for p in range(n, (n + 31) & ~31)], dtype=torch.int64, device=self.k[0].device)
            for vt in c.vt:
                vt.index_fill_(3, slots, 0)

    def _carry(self, c: "KVCache") -> "KVCache":
        c.length = self.length
        c.last_hidden = list(self.last_hidden)
        c._id_chunks = self._ids_carried()
        c.mask = self.mask
        c.side = dict(self.side)
        return c

    def fork(self) -> "KVCache":
        """An independent copy of the same capacity, with the same `ids`, `last_hidden`, mask and `side` entries (the tensors behind
        those are shared: nothing writes them in place): several continuations of one prefilled prefix, each on its own fork."""
        n_layers, B, H, hd, dev, dtype = self._geom
        c = KVCache(n_layers, B, H, hd, self.smax, dev, dtype, kv_dtype=self.kv_dtype)
        self._copy_into(c)
        return self._carry(c)

    def grow(self, smax: int) -> None:
        """Make room for `smax` positions (rounded up to 64) in place: new buffers, positions < length copied (one launch for all layers;
        V^T columns beyond the sequence zero, as in a fresh cache), the lists rebound, the pointer arrays and the reorder scratch dropped.
        smax below `length` is refused; a capacity the cache already has changes nothing."""
        smax = int(smax)
        if smax < self.length:
            raise ValueError(f"KVCache.grow({smax}): the cache holds {self.length} positions")
        if ((smax + 63) // 64) * 64 <= self.smax:
            return
        n_layers, B, H, hd, dev, dtype = self._geom
        c = KVCache(n_layers, B, H, hd, smax, dev, dtype, kv_dtype=self.kv_dtype)
        self._copy_into(c)
        self.smax = c.smax
        if self.kv_dtype is None:
            self.k, self.vt = c.k, c.vt
        else:
            self.k8, self.vt8, self.k_scale, self.vt_scale = c.k8, c.vt8, c.k_scale, c.vt_scale      # (the staging window has no pitch: kept)
            self._kv8_ptrs = None
        self._c_ptrs = None
        self._gather_scratch = None

    def gather_rows(self, parent, p0: int, p1: int) -> None:
        """Beam search's reorder: for every layer, positions [p0, p1) of row r of K and V^T become those of row parent[r] (int32 [B], device;
        HF's `beam_idx`).  The beams of an item share everything below the first generated position, so only that tail moves.  V^T moves in
        the whole 32-key blocks the range touches (`vt_slot`): what lies below p0 in the first block has to be equal in r and parent[r].
        A reorder in place would read rows it has overwritten under a swap, so the tail goes through a scratch the cache keeps (sized once,
        for every position from p0's block to the end): two launches for all layers (ops.kv_gather_rows), and a row with parent[r] == r
        moves no bytes.  The model-dtype caches only."""
        if self.kv_dtype is not None:
            raise NotImplementedError("KVCache.gather_rows: an fp8 cache is not reordered (its staging window would need its own treatment)")
        B, H, smax, hd, esz = self._shape()
        p0, p1 = int(p0), int(p1)
        if not 0 <= p0 <= p1 <= smax:
            raise ValueError(f"KVCache.gather_rows: [{p0}, {p1}) is not a range of positions of a cache of {smax}")
        if p1 == p0:
            return
        q0 = p0 & ~31
        sc = getattr(self, "_gather_scratch", None)
        if sc is None or sc[0] > q0:
            W, dev, dt, n = smax - q0, self.k[0].device, self.k[0].dtype, len(self.k)
            ks, vs = torch.empty(n, B, H, W, hd, device=dev, dtype=dt), torch.empty(n, B, H, hd, W, device=dev, dtype=dt)
            sc = self._gather_scratch = (q0, W, ks, vs, ops._ptr_array(list(ks)), ops._ptr_array(list(vs)))
        s0, W, _, _, sk, sv = sc
        ck, cv = self.c_ptrs()
        n = len(self.k)
        ops.kv_gather_rows(ck, cv, sk, sv, n, B, B, H, hd, esz, smax, W, p0, p0 - s0, p1 - p0, parent, parent)
        ops.kv_gather_rows(sk, sv, ck, cv, n, B, B, H, hd, esz, W, smax, p0 - s0, p0, p1 - p0, None, parent)

    def replicated(self, times: int, smax: int = None) -> "KVCache":
        """A cache of B * times rows whose rows r * times ... (r + 1) * times - 1 hold row r's positions (beam search: the prefill, vision
        tower included, runs once per item, not once per beam).  One launch for all layers; `last_hidden` is not carried."""
        if self.kv_dtype is not None:
            raise NotImplementedError("KVCache.replicated: an fp8 cache is not replicated")
        B, H, smax0, hd, esz = self._shape()
        c = KVCache(len(self.k), B * times, H, hd, smax0 if smax is None else smax, self.k[0].device, self.k[0].dtype)
        if self.length:
            row_map = torch.arange(B, device=self.k[0].device, dtype=torch.int32).repeat_interleave(times)
            ops.kv_gather_rows(*self.c_ptrs(), *c.c_ptrs(), len(self.k), B, B * times, H, hd, esz, smax0, c.smax, 0, 0, self.length, row_map, None)
        c.length = self.length
        return c

    def __len__(self):
        return len(self.k) if self.kv_dtype is None else len(self.k8)

    def to_legacy_cache(self):
        """The HF view of this cache (what `outputs.past_key_values` is in the reference under transformers 4.29.1, models/ullava_core.py:349-355):
        a tuple of per-layer (key, value) pairs, each [B, H, length, hd] with post-RoPE keys.  Pure data movement (a slice of the K buffer;
        the key-permuted V^T image gathered back into natural key order and transposed); `KVCache.from_hf` is the inverse.  An fp8 cache
        hands out its dequantized positions: it builds its bf16 twin (`dequantized()`, every layer at once) first, a transient allocation of
        about twice the fp8 cache's size; `__getitem__` dequantizes one layer only."""
        if self.kv_dtype is not None:
            return self.dequantized().to_legacy_cache()
        n = self.length
        idx = ops.vt_unpermute_index(self.smax).to(self.k[0].device)[:n]
        return tuple((k[:, :, :n].contiguous(), vt[..., idx].transpose(-1, -2).contiguous()) for k, vt in zip(self.k, self.vt))

    def __iter__(self):
        return iter(self.to_legacy_cache())

    def __getitem__(self, i):
        """layer i's (key, value) pair -- so that code written against a tuple of pairs (`past_key_values[0][0].shape[2]`, the idiom of
        4.29-era callers) reads this object too.  An fp8 cache dequantizes the layer."""
        if self.kv_dtype is not None:
            B, H, smax, hd = self.k8[i].shape
            k = torch.empty(B, H, max(self.length, 1), hd, device=self.k8[i].device, dtype=BF16)
            vt = torch.zeros(B, H, hd, smax, device=self.k8[i].device, dtype=BF16)
            if self.length:
                ops.dequantize_kv(*self.kv8_layer(i), self.length, k_out=k, vt_out=vt)
            idx = ops.vt_unpermute_index(smax).to(vt.device)[:self.length]
            return k[:, :, :self.length], vt[..., idx].transpose(-1, -2)
        n = self.length
        idx = ops.vt_unpermute_index(self.smax).to(self.k[i].device)[:n]
        return self.k[i][:, :, :n], self.vt[i][..., idx].transpose(-1, -2)

    @classmethod
    def from_hf(cls, past, headroom: int = DEFAULT_HEADROOM, kv_dtype=None):
        """A caller-supplied HF `past_key_values` -> KVCache (reference models/ullava_core.py:279-292 takes `past_key_values:
        Optional[List[torch.FloatTensor]]`): the legacy tuple of per-layer (key, value) pairs, each [B, H, S, hd] with post-RoPE keys, or a
        transformers Cache object exposing `key_cache` / `value_cache` lists (or `.layers[i].keys / .values`).  Keys are copied into the
        K buffers, values go through `ull_transpose_v` into the permuted V^T layout; `last_hidden` starts empty (hidden states of the
        cached positions are not part of an HF cache).  kv_dtype="fp8_e4m3": the keys and values are quantized into an fp8 cache."""
        if hasattr(past, "key_cache") and hasattr(past, "value_cache"):
            pairs = list(zip(past.key_cache, past.value_cache))
        elif hasattr(past, "layers"):
            pairs = [(l.keys, l.values) for l in past.layers]
        else:
            pairs = [(kv[0], kv[1]) for kv in past]
        if not pairs:
            raise ValueError("empty past_key_values")
        k0 = pairs[0][0]
        if k0.dim() != 4:
            raise ValueError("past_key_values entries must be [batch, heads, seq, head_dim] tensors")
        B, H, S, hd = k0.shape
        c = cls(len(pairs), B, H, hd, S + headroom, k0.device, k0.dtype, kv_dtype=kv_dtype)
        for li, (k, v) in enumerate(pairs):
            if k.shape != (B, H, S, hd) or v.shape != (B, H, S, hd):
                raise ValueError("past_key_values layers disagree in shape")
            if kv_dtype is not None:
                k, v = k.contiguous(), v.contiguous()
                ops.quantize_kv(k, k.stride()[:3], v, v.stride()[:3], *c.kv8_layer(li), 0, S)
                continue
            c.k[li][:, :, :S].copy_(k)
            vr = v.permute(0, 2, 1, 3).contiguous()                              # [B, S, H, hd]: heads contiguous per token (data movement)
            ops.transpose_v(vr, S * H * hd, H * hd, B, S, H, hd, pitch=c.smax, out=c.vt[li])
        c.length = S
        c._id_chunks = None                                        # an HF cache does not say what it was filled with
        return c

    @staticmethod
    def vt_slot(pos: int) -> int:
        """column of key `pos` inside V^T (32-key blocks stored as slot 8g+4a+r <- key 16a+4g+r, see transpose_v)."""
        w = pos & 31
        return (pos & ~31) + 8 * ((w >> 2) & 3) + 4 * (w >> 4) + (w & 3)
