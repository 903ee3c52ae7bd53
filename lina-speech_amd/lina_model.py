"""LinaModel: text embed + codec embed -> AttentiveRNN -> codec logits, with the
teacher-forced ``forward`` and the batched autoregressive ``generate_batch`` of the
reference (model/modeling_lina.py:14-192; same constructor, argument names, returns and
state-dict keys ``txt_embed / rvq_embed / logits_head / attentive_rnn / txt_encoder``).

MI355X-first differences that do not change results:
  * the text side of the cross-attention is projected once per utterance (prepare());
  * ``generate_batch`` runs the device-side loop by default (decode.DecodeEngine.generate: fused HIP step, 8 tokens per
    hipGraph replay): picks, stop bookkeeping, the attention log and the next-token embedding stay on the device, and the
    "all rows stopped" test is read back every ``stop_check_every`` steps instead of every step (the loop may run up to two
    such groups of extra steps; the returned tensors are trimmed to the exact length the reference would have produced);
  * the engine is cached per (batch, text length, weights) and re-armed for later calls (``clear_decode_cache``).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import ops
from .attentive import AttentiveRNN
from .codec import CodecHead, MultiEmbedding, topk_sampling, undelay_rvq


class LinaModel(nn.Module):
    def __init__(self, attentive_rnn: AttentiveRNN, d_model: int, n_quant: int, n_codebook: int,
                 n_special_token_in: int, n_special_token_out: int, n_txt_vocab: int, tie_embed: bool = False,
                 txt_encoder: Optional[nn.Module] = None, spk_encoder: Optional[nn.Module] = None,
                 mask_text_p: float = 0.0):
        super().__init__()
        if mask_text_p > 0.0:
            raise NotImplementedError("mask_text_p > 0 raises in the reference too (SURVEY App. D)")
        self.n_quant, self.n_codebook = n_quant, n_codebook
        self.n_special_token_in, self.n_special_token_out = n_special_token_in, n_special_token_out
        self.mask_text_p = mask_text_p
        self.n_txt_vocab = n_txt_vocab
        self.n_target_vocab = n_codebook + n_special_token_out
        self.txt_encoder, self.spk_encoder, self.attentive_rnn = txt_encoder, spk_encoder, attentive_rnn
        self.txt_embed = nn.Embedding(n_txt_vocab, d_model, padding_idx=0)
        self.rvq_embed = MultiEmbedding(n_quant, n_codebook + n_special_token_in, d_model, padding_idx=0)
        self.logits_head = CodecHead(n_quant, self.n_target_vocab, d_model)
        if tie_embed:
            self.logits_head.weight = self.rvq_embed.weight

    # ------------------------------------------------------------------ teacher-forced
    def forward(self, x, y, encoder_mask, crossatt_mask, logits_mask=None, attention_only=False,
                forced_attention=None, init_state=None, crossatt_pos=None, return_masked: bool = True):
        """Reference modeling_lina.py:72-108.  ``return_masked=False`` (ours): skip the two gathered outputs -- their
        boolean indexing has a data-dependent shape, i.e. a host sync, which a captured (hipGraph) train step cannot
        contain; the loss does not need them."""
        x_embd = self.txt_embed(x)
        # the LAST token's embedding is only ever read by the speaker encoder: without one, embed y[:, :-1] -- the values the
        # reference slices out of the full embedding (modeling_lina.py:80-84), minus the slice's copy forward and its
        # zero-fill + copy backward over [b, n, d]
        n_in = y.shape[1] - 1
        y_src = y if self.spk_encoder is not None else y[:, :-1]
        y_embd = self.rvq_embed(y_src.permute(2, 0, 1))               # 'b n q -> q b n' -> sum over q
        y_embd = y_embd.squeeze(0) if y_embd.shape[0] == 1 else y_embd.sum(0)   # (one quantizer: the sum of one term is a copy -- skipped)
        x_enc = self.txt_encoder(x_embd, mask=encoder_mask)
        if self.spk_encoder is not None:
            y_embd[:, 0] = self.spk_encoder(y_embd)
            y_embd = y_embd[:, :-1, :]
        y_hat, att = self.attentive_rnn(
            y_embd, x_enc, mask=crossatt_mask[:, :-1],
            forced_attention=None if forced_attention is None else forced_attention[:, :, :n_in],
            attention_only=attention_only, init_state=init_state, crossatt_pos=crossatt_pos)
        if attention_only:
            return att
        logits = self.logits_head(y_hat)
        target = y[:, 1:]
        if logits_mask is not None:
            keep = logits_mask[:, 1:]
            masked_logits = masked_target = None
            if return_masked:
                masked_logits, masked_target = logits[keep, :, :], target[keep, :]  # returned, as the reference does
            # the loss itself: masked positions carry the ignored class instead of being gathered out -- the same mean
            # over the same terms (reference modeling_lina.py:97-107), without the scatter of the gather in backward
            target = torch.where(keep.unsqueeze(-1), target, torch.ones_like(target))
        else:
            masked_logits, masked_target = logits, target
        loss = ops.cross_entropy(logits.reshape(-1, logits.shape[-1]), target.reshape(-1), ignore_index=1)   # K14
        return logits, loss, att, masked_logits, masked_target

    # ------------------------------------------------------------------ batched decode
    _ENGINE_CACHE_SIZE = 2
    # generate_batch(n_engines=None): from this many rows up the batch is decoded by TWO engines on two HIP streams (rows never
    # interact -- reference modeling_lina.py:125,152-179; measured at L169, ms per token as one / two engines: 512 rows 2.31 /
    # 2.16, 384 rows 1.82 / 1.74, 256 rows 1.38 / 1.36, 128 rows 0.875 / 0.852; 4 x 128 rows and every split of 64 rows are slower
    # than one engine: profiles/r06_two_engines.txt, r06_b64_engines.txt)
    AUTO_TWO_ENGINES_ROWS = 384

    def __getstate__(self):
        """copy.deepcopy / pickling: the cached decode engines (hipGraphs, static buffers) stay with the original."""
        st = self.__dict__.copy()
        st.pop("_decode_engines", None)
        return st

    def clear_decode_cache(self):
        """Drop the cached decode engines (packed weights, static buffers, captured hipGraphs) NOW.  Rarely needed for
        correctness: the cache key carries every parameter's (storage, version) AND a content fingerprint
        (``_weights_fingerprint``), so optimizer steps, ``load_state_dict``, writes through ``param.data`` and in-place
        writes to inference-mode parameters build a new engine by themselves."""
        for eng in self.__dict__.pop("_decode_engines", {}).values():
            eng.close()

    _FINGERPRINT_ELEMS = 4096

    def _weights_fingerprint(self):
        """Two numbers per parameter -- the L2 norm of its first ``_FINGERPRINT_ELEMS`` elements and of their positive part (the
        second one tells a sign flip apart) -- from multi-tensor kernels over views and one 8-byte-per-parameter read-back: the
        (storage, version) part of the cache key does not see ``param.data`` writes (EMA swaps, hand-edited weights) or in-place
        writes to parameters made under ``torch.inference_mode`` (no version counter), and a stale engine would silently decode
        with the old packed weights.  (A write that leaves the first 4096 elements of EVERY tensor, their storage and their
        version counters untouched is still missed: ``clear_decode_cache()`` after such surgery.)"""
        ps = [p.detach().reshape(-1)[:self._FINGERPRINT_ELEMS] for p in self.parameters()]
        if not ps:
            return ()
        stats = torch._foreach_norm(ps) + torch._foreach_norm(torch._foreach_clamp_min(ps, 0))
        return tuple(torch.stack(stats).float().cpu().tolist())

    def _decode_engine(self, x_enc: Tensor, B: int, init_state, n_engines: int = 1, state_dtype=None, x_lens=None):
        """The DecodeEngine of (batch size, text length, dtype, device, current weights), built once and re-armed for
        every later ``generate_batch`` call of the same shape: construction packs 0.3 GB of weights and captures two
        hipGraphs (~0.6 k kernel nodes), far more than a call at B = 64 should pay.  "Current weights" = every
        parameter's (storage, version) AND a content fingerprint (see ``_weights_fingerprint``).  ``x_lens`` (ragged
        text): an engine of the ragged step -- part of the key as a flag; the lengths themselves are re-armed in place."""
        from .decode import DecodeEngine, DecodeEngineGroup
        w = self.logits_head.weight
        key = (B, int(n_engines), int(x_enc.shape[1]), w.dtype, str(w.device), str(state_dtype),
               tuple((p.data_ptr(), -1 if p.is_inference() else p._version) for p in self.parameters()),
               self._weights_fingerprint()) + (("ragged",) if x_lens is not None else ())
        cache = self.__dict__.setdefault("_decode_engines", {})
        eng = cache.pop(key, None)
        if eng is None:
            if n_engines > 1:                                        # (no init_state / prompt in this form: the caller checked)
                eng = DecodeEngineGroup(self, x_enc, batch_size=B, n_engines=n_engines, state_dtype=state_dtype,
                                        x_lens=x_lens)
            else:
                eng = DecodeEngine(self, x_enc, batch_size=B, state_dtype=state_dtype,   # NotImplementedError: architecture
                                   x_lens=x_lens)                                         # not covered
                if init_state is not None:
                    eng.reset(state=init_state)
        elif n_engines > 1:
            eng.reset(x_enc, x_lens=x_lens)
        else:
            eng.reset(x_enc, state=init_state, x_lens=x_lens)
        cache[key] = eng                                             # most recently used last
        while len(cache) > self._ENGINE_CACHE_SIZE:
            cache.pop(next(iter(cache))).close()                     # an engine is a reference cycle: free its device memory now
        return eng

    @torch.inference_mode()
    def generate_batch(self, x: Tensor, batch_size: int = 3, prompt: Optional[Tensor] = None, device: str = "cpu",
                       max_seqlen: int = 1000, k: int = 100, first_greedy_quant: int = 1, temp: float = 1.0,
                       init_state=None, force_max_seqlen: bool = False, stop_check_every: int = 16,
                       engine: Optional[str] = None, seed: Optional[int] = None, n_engines: Optional[int] = None,
                       state_dtype: Optional[torch.dtype] = None, *, x_lens=None, prompt_lens=None):
        """Reference model/modeling_lina.py:111-192 (same arguments, same four returns).  ``engine``:
          None / "auto" -- the device-side loop (decode.DecodeEngine.generate: one hipGraph replay per 8 tokens, picks /
                           stop flags / attention log / next-token embedding inside the graph) when the architecture is
                           one it covers, else the module path;
          "loop"        -- the device-side loop or an error;   "fused" -- the fused step, one graph replay per token, picks
                           on the host side;   "module" -- ``AttentiveGLA.step`` + logits head per token (unfused).
        ``n_engines`` > 1 (device loop, no codec prompt, no init_state): the batch is cut into that many row ranges, one
        engine and one HIP stream each (decode.DecodeEngineGroup: at B = 512 two engines decode 6-8 % faster than one: one
        half's projections run under the other half's HBM-bound state update).  None (default): 2 from
        ``AUTO_TWO_ENGINES_ROWS`` rows up, else 1.  Greedy tokens do not depend on it (rows never interact, every kernel's
        per-row sums are independent of the row count); the sampled quantizers draw from a per-engine seed word.
        ``state_dtype`` (device loop, bf16 models; opt-in): ``torch.bfloat16`` keeps the recurrent state in bf16 and rounds it
        after every step, as the reference itself does for a bf16 model (model/gla.py:229-240 + Cache.update); default fp32.
        ``seed`` feeds the device-side sampler of the loop (default: drawn from torch's generator, so
        ``torch.manual_seed`` makes a call reproducible, like the reference's multinomial).
        ``x_lens`` (keyword only; ours): texts of different lengths in one batch -- ``x`` [B, Tmax] right-padded and row i's
        text ends at ``x_lens[i]`` (1 <= x_lens[i] <= Tmax; LongTensor or list).  ``x`` may also be a list of B 1-D texts
        (padded with 0 here, lengths derived; ``batch_size`` must equal len(x)).  Row i then decodes as
        ``generate_batch(x[i, :x_lens[i]], batch_size=1)`` would: the text encoder masks the padding, both attentions of the
        cross-attention run over the row's own positions with a positional table at its own width, the attention log holds
        zeros at the padding and row i's cut is trimmed to its text.  All lengths == Tmax: the uniform path, unchanged.
        ``prompt_lens`` (keyword only; ours): codec prompts of different lengths in one batch -- ``prompt`` [Q, B, P]
        right-padded and row i's excerpt ends at ``prompt_lens[i]`` (0 <= prompt_lens[i] <= P, 0 = no prompt; LongTensor or
        list).  ``prompt`` may also be a list of B tensors [Q, p_i] (padded here, lengths derived; ``batch_size`` must equal
        len(prompt)).  Row i then decodes as ``generate_batch(x_i, batch_size=1, prompt=prompt[:, i:i+1, :p_i])`` would: the
        reference's ``t < p_len`` rule (modeling_lina.py:175) with the row's own p_len.  The min(prompt_lens) + 1 positions
        common to every row go through the one-pass prefill; from there the loop feeds each row its prompt token while it has
        one (K6f on the device loop, ``torch.where`` on the other paths).  All lengths == P: the uniform path, unchanged.  No
        speaker encoder (the reference's reads the first frames of the prompt with no mask)."""
        B, Q = batch_size, self.n_quant
        prompt, p_lens = self._ragged_prompt(prompt, B, prompt_lens)
        if p_lens is not None and self.spk_encoder is not None:
            raise NotImplementedError("prompt_lens with a speaker encoder: it reads the padded prompt with no mask")
        x, lens = self._ragged_text(x, B, x_lens)
        x = (x.unsqueeze(0).expand(B, -1) if x.dim() == 1 else x).to(device)   # 1-D: one text for every row
        enc_mask = cross_mask = None
        if lens is not None:                                    # the reference's collate masks (initial_state.py:65-70)
            live = torch.arange(x.shape[1], device=device)[None, :] < lens.to(device)[:, None]             # [B, Tmax]
            enc_mask = live[:, None, :] & live[:, :, None]
            cross_mask = live[:, None, :]                                                                   # [B, 1, Tmax]
        x_enc = self.txt_encoder(self.txt_embed(x), mask=enc_mask)
        y_embd = self.rvq_embed.embed_sum(torch.ones(Q, B, 1, dtype=torch.long, device=device))

        p_len = -1
        prompt_tok = None
        if prompt is not None:
            if prompt.shape[1] != B:
                prompt = prompt.expand(Q, B, -1) + 3
            prompt_tok = prompt.to(device)
            prompt = self.rvq_embed.embed_sum(prompt_tok)
            p_len = prompt.shape[1]
            if self.spk_encoder is not None:
                prompt[:, 0] = self.spk_encoder(prompt)

        # prompts of different lengths: positions 0 .. min(p) are common to every row (the prefill below, as for one p_len);
        # from there row b is fed prompt[b, t] while t < p_b -- `fed(t, picks)` is the reference's line 175 per row
        p_dev = None
        if p_lens is not None:
            p_dev = p_lens.to(device)
            p_len = int(p_lens.min())

        def fed(t, q_sampled):
            if prompt is None or (p_dev is None and t >= p_len):
                return self.rvq_embed.embed_sum(q_sampled)
            if p_dev is None:
                return prompt[:, [t]]
            if t >= prompt.shape[1]:
                return self.rvq_embed.embed_sum(q_sampled)
            return torch.where((t < p_dev)[:, None, None], prompt[:, [t]], self.rvq_embed.embed_sum(q_sampled))

        mode = engine or "auto"
        if mode not in ("auto", "loop", "fused", "module"):
            raise ValueError("engine must be None, 'auto', 'loop', 'fused' or 'module'")
        eng = None
        if mode in ("auto", "loop"):
            if n_engines is None:
                n_engines = 2 if B >= self.AUTO_TWO_ENGINES_ROWS else 1
            n_eng = n_engines if (n_engines > 1 and prompt is None and init_state is None and B >= 2 * n_engines) else 1
            try:
                eng = self._decode_engine(x_enc, B, init_state, n_eng, state_dtype, x_lens=lens)
            except NotImplementedError:
                if mode == "loop":
                    raise
                mode = "module"
        if eng is not None and not hasattr(eng, "state"):            # a group of engines: no prompt, nothing to prefill
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)))
            qs, atts, n = eng.generate(max_seqlen, y_embd, k=k, temp=temp, first_greedy_quant=first_greedy_quant, seed=seed,
                                       force_max_seqlen=force_max_seqlen, stop_check_every=stop_check_every, log_att=True)
            return self._finish_generate(qs, atts, (qs == 2).all(dim=0), B, device, lens)
        # (ragged text: the module path and the prompt prefill need the per-row positional tables of prepare(lens=))
        ragged_prepared = None if lens is None else self.attentive_rnn.cross_att.prepare(x_enc, lens=lens)
        if eng is not None:
            state, prepared, step_fn = eng.state, ragged_prepared, None
        elif mode == "fused":
            from .decode import DecodeEngine
            step_fn = DecodeEngine(self, x_enc, batch_size=B, state=init_state, x_lens=lens)
            state = step_fn.state
            prepared = ragged_prepared
        else:
            state = init_state if init_state is not None else self.attentive_rnn.init_state(
                max_seqlen=max_seqlen, batch_size=B)
            prepared = ragged_prepared if lens is not None else self.attentive_rnn.cross_att.prepare(x_enc)

            def step_fn(y, t):
                h, att, _ = self.attentive_rnn.step(y, x_enc, t, state, prepared=prepared, crossatt_mask=cross_mask)
                return self.logits_head(h), att

        # ---- prompt prefill: the reference feeds the start token and the p_len prompt tokens one step at a time
        # (modeling_lina.py:152-176); their inputs are known in advance, so all p_len + 1 positions go through the stack in
        # ONE teacher-forced pass on the cached path (K2 chunk scan + conv prefill + cached pos_net block, the same
        # recurrence as p_len + 1 single steps) and the per-position bookkeeping below consumes its logits.
        pre_logits = pre_att = None
        n_pre = 0
        if prompt is not None and p_len > 0 and hasattr(self.attentive_rnn, "step"):
            n_pre = min(p_len + 1, max_seqlen)
            y_seq = torch.cat([y_embd, prompt[:, :n_pre - 1]], dim=1)
            h, pre_att, _ = self.attentive_rnn.step(y_seq, x_enc, 0, state, prepared=prepared,
                                                    crossatt_mask=None if cross_mask is None else cross_mask.expand(-1, n_pre, -1))
            pre_logits = self.logits_head(h)                        # [B,n_pre,Q,L]

        def pick_tokens(logits):                                    # [B,1,Q,L] -> [Q,B,1]
            per_q = logits.squeeze(1).transpose(0, 1)               # [Q,B,L]
            return torch.stack([topk_sampling(per_q[i], k=k, temp=temp) if i < first_greedy_quant
                                else topk_sampling(per_q[i], k=1) for i in range(Q)])

        if eng is not None:
            # ---- the device-side loop: the prefill's positions are picked here and filed in front of it
            preload = None
            y0 = y_embd
            if n_pre > 0:
                pre_q = torch.cat([pick_tokens(pre_logits[:, t:t + 1]) for t in range(n_pre)], dim=2)   # [Q,B,n_pre]
                preload = (pre_q, pre_att)
                y0 = fed(n_pre - 1, pre_q[:, :, -1:])          # (one p_len: the prompt token if n_pre - 1 < p_len, else the pick's)
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)))
            qs, atts, n = eng.generate(max_seqlen, y0, k=k, temp=temp, first_greedy_quant=first_greedy_quant, seed=seed,
                                       force_max_seqlen=force_max_seqlen, stop_check_every=stop_check_every,
                                       log_att=True, preload=preload,
                                       forced=None if p_lens is None else (prompt_tok, p_lens))
            return self._finish_generate(qs, atts, (qs == 2).all(dim=0), B, device, lens)

        all_stop = torch.zeros(B, 1, dtype=torch.bool, device=device)
        qs, atts, stop_tokens = [], [], []
        stop_at = None                      # first step index at which every row had stopped
        for t in range(max_seqlen):
            if t < n_pre:
                logits, att = pre_logits[:, t:t + 1], pre_att[:, :, t:t + 1]
            else:
                logits, att = step_fn(y_embd, t)                # [B,1,Q,L], [B,2,1,Ttxt]
            atts.append(att)
            q_sampled = pick_tokens(logits)                     # [Q,B,1]
            qs.append(q_sampled)
            is_stop = (q_sampled == 2).all(dim=0)               # every quantizer emitted the stop token
            stop_tokens.append(is_stop)
            all_stop |= is_stop
            if not force_max_seqlen and ((t + 1) % stop_check_every == 0 or t == max_seqlen - 1):
                flags = torch.stack([s.squeeze(-1) for s in stop_tokens]).cumsum(0).bool().all(dim=1)  # [t+1]
                if bool(flags.any()):
                    stop_at = int(torch.nonzero(flags)[0])
                    break
            y_embd = fed(t, q_sampled)

        if stop_at is not None:             # trim to what a per-step check would have produced
            qs, atts, stop_tokens = qs[:stop_at + 1], atts[:stop_at + 1], stop_tokens[:stop_at + 1]
        atts = torch.cat(atts, dim=2) if atts[0] is not None else None
        qs = torch.stack(qs, dim=2).squeeze(-1)                                  # [Q,B,n]
        return self._finish_generate(qs, atts, torch.cat(stop_tokens, dim=1), B, device, lens)

    # ------------------------------------------------------------------ queue decode: finished rows take the next text
    def generate_stream(self, texts, batch_size: int, max_seqlen=1000, k: int = 100, first_greedy_quant: int = 1,
                        temp: float = 1.0, seed: Optional[int] = None, stop_check_every: int = 16,
                        state_dtype: Optional[torch.dtype] = None, device: str = "cpu", max_text_len: Optional[int] = None,
                        prompt=None, init_state=None):
        """Decode a QUEUE of N texts on ``batch_size`` rows (ours; the device-side loop only): a row whose utterance has
        stopped -- or reached its step cap -- is re-armed with the next queued text between two graph replays while the other
        rows go on (decode.DecodeEngine.serve, K6g), instead of stepping on until the slowest row of its batch has stopped.
        A generator yielding ``(i, codes, att)`` as utterances finish (not in queue order).

        ``texts``: N 1-D LongTensors; ``max_seqlen``: an int or N ints, the step cap of each utterance.  ``(codes, att)`` of
        utterance i is ``cuts[0]`` of ``generate_batch(texts[i], batch_size=1, max_seqlen=cap_i, ...)``: the reference's
        post-processing (``_finish_generate``) of the row's own steps, trimmed to its first stop step + 1 or its cap.  Greedy
        results (k = 1 or first_greedy_quant = 0) do not depend on ``batch_size``, on the queue order or on
        ``stop_check_every``.  SAMPLED results are reproducible for a fixed (seed, batch_size, order, stop_check_every) but are
        NOT those of the alone run: the draws hash (seed, step of the loop, row), and an utterance's row and start step depend
        on the queue.  Utterances start on window boundaries at the loop's checks: a row idles up to 2 * ``every`` steps
        between two utterances (``every`` = stop_check_every rounded up to a multiple of max(8, window)).
        The texts are encoded in refill batches of one fixed row count (min(batch_size, 32), padded) under the ragged masks,
        so that an utterance's result, bit for bit, does not depend on which others were refilled with it; the engine is the
        cached ragged engine of (batch_size, ``max_text_len`` or the longest text).  With N < batch_size the spare rows idle
        from the start.
        ``prompt``, ``init_state``, a speaker encoder and an architecture the engine does not cover raise
        NotImplementedError: there is no fallback to the module path."""
        if prompt is not None or init_state is not None:
            raise NotImplementedError("generate_queue: codec prompts and start states for refilled rows are not built")
        if self.spk_encoder is not None:
            raise NotImplementedError("generate_queue: no speaker encoder")
        texts = list(texts)
        n_utts = len(texts)
        if any((not isinstance(t, Tensor)) or t.dim() != 1 or t.shape[0] < 1 for t in texts):
            raise ValueError("texts: a list of non-empty 1-D LongTensors")
        caps = [int(max_seqlen)] * n_utts if isinstance(max_seqlen, int) else [int(c) for c in max_seqlen]
        if len(caps) != n_utts or any(c < 1 for c in caps):
            raise ValueError(f"max_seqlen: an int or one step cap >= 1 per text ({n_utts})")
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        lens_all = [int(t.shape[0]) for t in texts]
        Tn = int(max_text_len) if max_text_len else max(lens_all, default=1)
        if lens_all and max(lens_all) > Tn:
            raise ValueError(f"a text is longer than max_text_len = {Tn}")
        return self._queue_gen(texts, lens_all, caps, batch_size, Tn, k, first_greedy_quant, temp, seed, stop_check_every,
                               state_dtype, device)

    @torch.inference_mode()
    def _queue_gen(self, texts, lens_all, caps, B, Tn, k, first_greedy_quant, temp, seed, stop_check_every, state_dtype,
                   device):
        if not texts:
            return
        w = self.logits_head.weight
        idle = torch.zeros(B, Tn, self.txt_embed.weight.shape[1], dtype=w.dtype, device=device)
        eng = self._decode_engine(idle, B, None, 1, state_dtype, x_lens=torch.ones(B, dtype=torch.long))
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)))

        def encode(ids, m):                                  # a refill batch through the text encoder, ragged masks: always
            x = torch.zeros(m, Tn, dtype=torch.long, device=device)      # m rows (padding: one-token texts), so that an
            for r, i in enumerate(ids):                                  # utterance's text side does not depend on how many
                x[r, :lens_all[i]] = texts[i].to(device)                 # rows were free with it
            lens = [lens_all[i] for i in ids] + [1] * (m - len(ids))
            ln = torch.tensor(lens, device=device)
            live = torch.arange(Tn, device=device)[None, :] < ln[:, None]
            return self.txt_encoder(self.txt_embed(x), mask=live[:, None, :] & live[:, :, None]), lens

        def finish(i, qs, atts, txt_len):
            cuts = self._finish_generate(qs, atts, (qs == 2).all(dim=0), 1, device, torch.tensor([txt_len]))[3]
            return i, cuts[0][0], cuts[0][1]

        yield from eng.serve(caps, encode, finish, k=k, temp=temp, first_greedy_quant=first_greedy_quant, seed=seed,
                             stop_check_every=stop_check_every)

    def generate_queue(self, texts, batch_size: int, max_seqlen=1000, k: int = 100, first_greedy_quant: int = 1,
                       temp: float = 1.0, seed: Optional[int] = None, stop_check_every: int = 16,
                       state_dtype: Optional[torch.dtype] = None, device: str = "cpu", max_text_len: Optional[int] = None,
                       prompt=None, init_state=None):
        """``generate_stream`` collected: N pairs ``(codes, att)`` in queue order ([] for an empty queue)."""
        texts = list(texts)
        out = [None] * len(texts)
        for i, codes, att in self.generate_stream(texts, batch_size, max_seqlen=max_seqlen, k=k,
                                                  first_greedy_quant=first_greedy_quant, temp=temp, seed=seed,
                                                  stop_check_every=stop_check_every, state_dtype=state_dtype, device=device,
                                                  max_text_len=max_text_len, prompt=prompt, init_state=init_state):
            out[i] = (codes, att)
        return out

    @torch.inference_mode()
    def synthesize(self, texts, vocoder, batch_size: int, *, vocoder_batch: int = 32, bandwidth_id=None,
                   **generate_queue_kwargs):
        """Texts in, waveforms out (ours): ``generate_stream`` feeding the ragged vocoder.  N 1-D waveforms in queue order,
        utterance i's being ``vocoder(codes_i, bandwidth_id)`` of its own codes alone (``codes_i`` as ``generate_queue``
        returns them, ``len(codes_i) * hop`` samples).  Finished utterances are collected, sorted by length and vocoded
        ``vocoder_batch`` at a time with their lengths (``WavTokenizerDecoder.forward(..., lens=...)``), which bounds the
        padding of a group by the spread of neighbouring lengths.  An utterance whose cut holds no code gives an empty
        waveform and is not sent to the vocoder.  ``vocoder.n_codes`` must cover the model's ``n_codebook``; the restrictions
        of ``generate_stream`` apply (no prompt, no start state, no speaker encoder)."""
        if vocoder_batch < 1:
            raise ValueError("vocoder_batch must be >= 1")
        if vocoder.n_codes < self.n_codebook:
            raise ValueError(f"the vocoder knows {vocoder.n_codes} codes, the model emits {self.n_codebook}")
        texts = list(texts)
        codes = [None] * len(texts)
        for i, c, _ in self.generate_stream(texts, batch_size, **generate_queue_kwargs):
            codes[i] = c
        return self.vocode(codes, vocoder, vocoder_batch=vocoder_batch, bandwidth_id=bandwidth_id)

    @staticmethod
    @torch.inference_mode()
    def vocode(codes, vocoder, *, vocoder_batch: int = 32, bandwidth_id=None):
        """The second half of ``synthesize``: N code cuts ``[Q, 1, n_i]`` (or ``[Q, n_i]``; as ``generate_queue`` returns them)
        -> N 1-D waveforms of ``n_i * hop`` samples in the same order, through the ragged vocoder in groups of
        ``vocoder_batch`` utterances sorted by length; an empty cut gives an empty waveform without a vocoder call."""
        if vocoder_batch < 1:
            raise ValueError("vocoder_batch must be >= 1")
        w = vocoder.head.istft.window
        codes = [c[:, 0] if c.dim() == 3 else c for c in codes]            # [Q, n_i]
        out = [torch.zeros(0, dtype=torch.float32, device=w.device) for _ in codes]
        order = sorted((i for i, c in enumerate(codes) if c.shape[-1] > 0), key=lambda i: codes[i].shape[-1])
        for lo in range(0, len(order), vocoder_batch):
            ids = order[lo:lo + vocoder_batch]
            for i, wav in zip(ids, vocoder([codes[i].to(w.device) for i in ids], bandwidth_id)):
                out[i] = wav
        return out

    @staticmethod
    def _ragged_text(x, B: int, x_lens):
        """generate_batch's text argument -> (x, lengths [B] LongTensor or None).  A list of B 1-D texts is right-padded with
        0 and its lengths derived; lengths that are all the padded width mean a uniform batch (None: today's path)."""
        from .decode import text_lengths
        if isinstance(x, (list, tuple)):
            if x_lens is not None:
                raise ValueError("x_lens: the list form of x carries its own lengths")
            if len(x) != B:
                raise ValueError(f"x is a list of {len(x)} texts: batch_size must equal it (got {B})")
            if any(t.dim() != 1 for t in x):
                raise ValueError("x as a list: one 1-D LongTensor per row")
            x_lens = [int(t.shape[0]) for t in x]
            if min(x_lens) < 1:
                raise ValueError("every text length must be >= 1")
            x = torch.nn.utils.rnn.pad_sequence([t.to(x[0].device) for t in x], batch_first=True, padding_value=0)
        if x_lens is None:
            return x, None
        if x.dim() != 2:
            raise ValueError("x_lens needs x as [B, Tmax] right-padded texts (a 1-D x is one text for every row)")
        if x.shape[0] != B:
            raise ValueError(f"x has {x.shape[0]} rows for batch_size {B}")
        lens = torch.tensor(text_lengths(x_lens, B, x.shape[1]), dtype=torch.long)
        return x, (None if bool((lens == x.shape[1]).all()) else lens)

    @staticmethod
    def _ragged_prompt(prompt, B: int, prompt_lens):
        """generate_batch's prompt argument -> (prompt, lengths [B] LongTensor or None).  A list of B prompts [Q, p_i] is
        right-padded with 0 and its lengths derived; lengths that are all the padded width mean one p_len (None: today's
        path)."""
        from .decode import prompt_lengths
        if isinstance(prompt, (list, tuple)):
            if prompt_lens is not None:
                raise ValueError("prompt_lens: the list form of prompt carries its own lengths")
            if len(prompt) != B:
                raise ValueError(f"prompt is a list of {len(prompt)} excerpts: batch_size must equal it (got {B})")
            if any(p.dim() != 2 or p.shape[0] != prompt[0].shape[0] for p in prompt):
                raise ValueError("prompt as a list: one LongTensor [Q, p_i] per row")
            prompt_lens = [int(p.shape[1]) for p in prompt]
            P = max(prompt_lens)
            padded = torch.zeros(prompt[0].shape[0], B, P, dtype=torch.long, device=prompt[0].device)
            for i, p in enumerate(prompt):
                padded[:, i, :p.shape[1]] = p
            prompt = padded
        if prompt_lens is None:
            return prompt, None
        if prompt is None:
            raise ValueError("prompt_lens needs a prompt")
        if prompt.dim() != 3 or prompt.shape[1] != B:
            raise ValueError(f"prompt_lens needs prompt as [Q, B, P] right-padded excerpts, one per row (B = {B}): the "
                             "broadcast (+3) rule belongs to the one-prompt form")
        lens = torch.tensor(prompt_lengths(prompt_lens, B, prompt.shape[2]), dtype=torch.long)
        return prompt, (None if bool((lens == prompt.shape[2]).all()) else lens)

    def _finish_generate(self, qs, atts, is_stop, B, device, lens=None):
        """Post-processing of the reference (modeling_lina.py:180-192) from the [B,n] stop flags: the stop-flag matrix
        with the closing column of ones, the un-delayed codes and the per-row cuts.  The reference takes
        ``torch.unique(stop_idx[i])[1]`` row by row (a sort and a host read per row); the set it sorts is {0} plus the
        positions of the row's stop flags, so element [1] is the first position >= 1 that carries a flag -- computed here
        for all rows at once and read back once.  ``lens`` (ragged text): row i's attention cut ends at its own text."""
        stop_tokens = torch.cat([is_stop.float(), torch.ones(B, 1, device=device)], dim=1)    # [B,n+1]
        n = stop_tokens.shape[1]
        rvq = (undelay_rvq(qs) - self.n_special_token_in).clamp_min(0)
        pos = torch.arange(n, device=device)[None, :].expand(B, -1)
        flagged = (stop_tokens != 0) & (pos >= 1)
        if n < 2:
            raise IndexError("generate_batch: no step was decoded (max_seqlen == 0)")   # the reference's unique()[1] raises too
        first = torch.where(flagged, pos, torch.full_like(pos, n)).min(dim=1).values.tolist()
        txt = [None] * B if lens is None else lens.tolist()
        cuts = [(rvq[:, i:i + 1, :idx - self.n_quant], None if atts is None else atts[i, :, :idx, :txt[i]])
                for i, idx in enumerate(first)]
        return qs, atts, stop_tokens, cuts
