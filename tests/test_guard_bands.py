"""Every kernel family under guard bands (tests/guard.py): an existing case function runs UNCHANGED -- its shapes, assertions
and tolerances are its own -- while its inputs, the tensors it hands the kernels to write and the outputs the launchers allocate
themselves sit between NaN-filled (integers: 1-filled) bands.  A case passes when
  * its own assertions hold: outputs finite and at parity although every input is followed and preceded by NaN (a load past
    the end of an input that reaches the arithmetic would show), and every ``empty`` output starts out as NaN;
  * every band is bit-identical to its fill afterwards (a store past either end of a tensor would show);
  * the arena really held the case's tensors: at least ``n_case`` allocated by the case function and ``n_lib`` by the launchers
    (both counted by reading the case: the operands it puts on the device plus the outputs of its launches, a lower bound that
    a refactor cannot silently empty).
The shapes are the smallest of the existing argument lists at which tails exist.  The same list runs on the CPU emulator and,
under ``-m gpu``, on the device, where a few paths are added that the emulator cannot exercise faithfully (GPU_ONLY).
What the arena does not guard is listed in the docstring of tests/guard.py."""
import pytest
import torch

import kernel_cases as KC
import lina_speech_amd.kernels as LK
import prompt_cases as PC
import ragged_cases as RC
from guard import BAND, GuardArena, GuardDamage, guarded
from test_k1w_persist import check_persist_equals_plain

F32, BF16 = torch.float32, torch.bfloat16


# ----------------------------------------------------------------------------- the harness itself
@pytest.mark.parametrize("dtype", [F32, BF16, torch.int64, torch.int32])
def test_arena_layout_and_fill(dtype):
    arena = GuardArena("cpu")
    t = arena.empty((3, 5), dtype, label="probe")
    buf, start, nbytes = arena.raw(t)
    assert t.data_ptr() % 256 == 0 and t.data_ptr() == buf.data_ptr() + start and nbytes == 15 * t.element_size()
    assert start >= BAND and buf.numel() - start - nbytes >= BAND >= 4096          # the back band starts right behind the tensor
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all()) and bool((buf == 0xFF).all())
    else:
        assert bool((t == 1).all()) and bool((buf.view(dtype) == 1).all())
    p = arena.place(torch.arange(24).view(2, 3, 4).to(dtype).transpose(1, 2))
    assert p.shape == (2, 4, 3) and p.stride() == (12, 1, 4) and torch.equal(p, torch.arange(24).view(2, 3, 4).to(dtype).transpose(1, 2))
    z = arena.empty((0, 7), dtype)
    assert arena.raw(z)[2] == 0 and arena.count == 3
    arena.check()


@pytest.mark.parametrize("dtype", [F32, BF16, torch.int64])
@pytest.mark.parametrize("side", ["back", "front"])
def test_arena_check_names_tensor_side_and_offset(dtype, side):
    """A host-side write of one element just past (just before) a guarded tensor, made through the arena's own buffer (it stays
    inside one allocation; no kernel is involved), fails check() with the right tensor, side, offset and byte count."""
    arena = GuardArena("cpu")
    a = arena.empty((4, 6), dtype, label="bystander")
    t = arena.place(torch.zeros(7, 3).to(dtype), label="victim")
    arena.check()
    buf, start, nbytes = arena.raw(t)
    item = t.element_size()
    assert nbytes == 21 * item
    elems = buf.view(dtype)
    at = (start + nbytes) // item if side == "back" else start // item - 1
    elems[at] = 0                                               # 0 differs from NaN and from 1 in every byte that is not 0 already
    changed = item if dtype.is_floating_point else 1           # (the integer 1 has one non-zero byte)
    off = nbytes if side == "back" else -item
    with pytest.raises(GuardDamage) as e:
        arena.check()
    msg = str(e.value)
    assert f"{side} band of tensor (7, 3) {str(dtype)[6:]} [victim]" in msg and "bystander" not in msg, msg
    assert f"{changed} damaged byte(s), the first at byte offset {off} " in msg, msg
    assert torch.equal(t, torch.zeros(7, 3).to(dtype)) and a.shape == (4, 6)


def test_guarded_routes_and_restores(monkeypatch):
    real_to, real_clone = torch.Tensor.to, torch.Tensor.clone
    with guarded(monkeypatch, "cpu") as arena:
        assert KC.torch is not torch and LK.torch is KC.torch
        x = torch.randn(3, 4)
        y = x.to("cpu")
        assert y is not x and arena.owns(y) and torch.equal(x, y) and y.to("cpu") is y
        assert arena.owns(y.clone()) and not arena.owns(x.clone()) and not arena.owns(y.to(torch.float64))
        assert arena.owns(KC.torch.zeros(2, 2, device="cpu")) and not arena.owns(KC.torch.zeros(2, 2))
        e = KC.torch.empty(5, dtype=BF16, device="cpu")
        assert arena.owns(e) and bool(torch.isnan(e).all())
        assert arena.owns(KC.torch.full_like(y, 2.0)) and KC.torch.float32 is torch.float32
        leaf = x.clone().requires_grad_()
        assert not arena.owns(leaf.to("cpu")) and arena.count == 5
        w = torch.randn(5, 32)
        assert arena.owns(KC.ops.pack_rows(w)) and torch.equal(KC.ops.unpack_rows(KC.ops.pack_rows(w), 5, 32), w)
        arena.check()
    assert KC.torch is torch and LK.torch is torch and KC.ops.pack_rows is LK.pack_rows
    assert torch.Tensor.to is real_to and torch.Tensor.clone is real_clone


# ----------------------------------------------------------------------------- the cases
def _ragged(dev, monkeypatch, d, dtype, shared_pe):
    # the three ragged cross-attention launches at the lengths of the ragged decode tests: (13, 40, 1, 64) in T_txt = 64
    monkeypatch.setattr(RC, "ragged_lens", lambda B, Tmax: list(RC.RAGGED_LENS))
    RC.check_ragged_kernels(dev, len(RC.RAGGED_LENS), d, dtype, Tmax=64, shared_pe=shared_pe)


def _wide_split_k(dev, monkeypatch, nw):
    monkeypatch.setenv("LINA_SKINNY_WAVES", str(nw))
    KC.check_linear_skinny_packed(dev, 20, 48, 1024, BF16, ln=False, bias=False, resid=True)
    KC.check_inproj_packed(dev, 9, 1024, 32, 32, BF16)


def _k2b_generic_bf16(dev, monkeypatch):
    monkeypatch.setattr(KC.ops.POLICY, "k2b_path", "sweeps")
    KC.check_chunk_bwd(dev, B=1, H=1, T=40, Dk=64, Dv=64, dtype=BF16)


_TALL = [(130, 70, 160, BF16, False, True, True, 0), (70, 100, 96, BF16, True, True, False, 0),
         (129, 56, 288, BF16, True, True, False, 40), (33, 64, 128, BF16, False, False, False, 64),
         (140, 48, 80, F32, True, True, True, 0), (20, 40, 48, F32, True, False, False, 21)]


def _tall(i, variant):
    M, N, K, dtype, ln, bias, resid, sw = _TALL[i]
    return lambda dev, mp: KC.check_linear_tall(dev, M, N, K, dtype, ln=ln, bias=bias, resid=resid, swiglu=sw, variant=variant)


def C(name, fn, n_case, n_lib=0):
    return pytest.param(fn, n_case, n_lib, id=name)


# (id, case(dev, monkeypatch), least number of guarded tensors the case function itself creates, least number the launchers create)
# n_case: operands put on the device + buffers handed to the kernels, as read off the case function (a lower bound);
# n_lib: outputs / workspaces ``lina_speech_amd`` allocates for the launches of the case (0: the case passes every output in).
CASES = [
    # K1 recurrent: q k v gk h0 + a cloned state | o S, o (h0=None), o (state in place) (bf16: + o S with fp32 gates)
    C("k1-f32", lambda d, mp: KC.check_recurrent(d, B=2, H=2, T=3, Dk=128, Dv=64, dtype=F32), 6, 4),
    C("k1-bf16", lambda d, mp: KC.check_recurrent(d, B=2, H=2, T=2, Dk=64, Dv=64, dtype=BF16), 6, 6),
    # K2 chunk: 5 operands | o, S of chunk_gla, fused_chunk_gla, the h0=None call and K1
    C("k2-generic-f32", lambda d, mp: KC.check_chunk(d, B=1, H=2, T=37, Dk=64, Dv=64, dtype=F32), 5, 7),
    C("k2-generic-bf16", lambda d, mp: KC.check_chunk(d, B=1, H=2, T=33, Dk=64, Dv=64, dtype=BF16), 5, 7),
    C("k2-generic-resets", lambda d, mp: KC.check_chunk(d, B=1, H=1, T=40, Dk=64, Dv=64, dtype=F32, resets=True), 5, 7),
    C("k2-full-head-T33", lambda d, mp: KC.check_chunk(d, B=1, H=1, T=33, Dk=256, Dv=256, dtype=BF16), 5, 7),
    C("k2-full-head-T70-resets", lambda d, mp: KC.check_chunk(d, B=1, H=1, T=70, Dk=256, Dv=256, dtype=BF16, resets=True), 5, 7),
    C("k2-head-groups-4x64", lambda d, mp: KC.check_chunk(d, B=1, H=4, T=45, Dk=64, Dv=64, dtype=BF16), 5, 7),
    C("k2-head-groups-2x128", lambda d, mp: KC.check_chunk(d, B=1, H=2, T=70, Dk=128, Dv=128, dtype=BF16, resets=True), 5, 7),
    # segment-parallel: o S + the boundary-state workspace (kept for the later launches), o S of the plain kernel, o (h0=None)
    C("k2-segments-T100-n3", lambda d, mp: KC.check_chunk_segmented(d, B=1, H=1, T=100, nseg=3), 5, 6),
    C("k2-segments-T70-n2-resets", lambda d, mp: KC.check_chunk_segmented(d, B=1, H=1, T=70, nseg=2, resets=True), 5, 6),
    C("k2-segments-head-groups", lambda d, mp: KC.check_chunk_segmented(d, B=1, H=4, T=70, nseg=2, resets=True, D=64), 5, 6),
    C("k2-value-column-blocks", lambda d, mp: KC.check_chunk(d, B=1, H=1, T=40, Dk=256, Dv=512, dtype=BF16, resets=True), 5, 7),
    # K2b: 5 operands, d_o, d_ht, 4 leaf clones + the h0 leaf | forward o, S + dq dk dv dg dh0
    C("k2b-generic-f32", lambda d, mp: KC.check_chunk_bwd(d, B=1, H=2, T=37, Dk=64, Dv=64, dtype=F32), 11, 6),
    C("k2b-generic-bf16", _k2b_generic_bf16, 11, 6),
    C("k2b-generic-no-state", lambda d, mp: KC.check_chunk_bwd(d, B=1, H=1, T=40, Dk=64, Dv=64, dtype=F32, resets=True,
                                                               with_h0=False, with_dht=False), 9, 4),
    C("k2b-value-column-blocks", lambda d, mp: KC.check_chunk_bwd(d, B=1, H=1, T=40, Dk=256, Dv=512, dtype=BF16, resets=True), 11, 6),
    # the full-head sweeps called directly: 5 operands, d_o (, d_ht) | (o, ht of the forward) + dq|dk|dv in one buffer, dg,
    # scratch (, dh0)
    C("k2b-full-T33", lambda d, mp: KC.check_chunk_bwd_full(d, 1, 1, 33, 256, 1, with_h0=True, with_dht=True), 7, 6),
    C("k2b-full-T40-no-state", lambda d, mp: KC.check_chunk_bwd_full(d, 1, 1, 40, 256, 1, with_h0=False, with_dht=False), 5, 3),
    C("k2b-full-T100-n3", lambda d, mp: KC.check_chunk_bwd_full(d, 1, 1, 100, 256, 3, with_h0=True, with_dht=True), 7, 6),
    C("k2b-full-head-groups", lambda d, mp: KC.check_chunk_bwd_full(d, 1, 4, 70, 64, 2, resets=True), 7, 6),
    # simple GLA: 5 operands | o, S (fp32 also: the backward)
    C("simple-gla-f32", lambda d, mp: KC.check_chunk_simple(d, B=1, H=2, T=37, Dk=64, Dv=64, dtype=F32, with_h0=True), 5, 2),
    C("simple-gla-bf16", lambda d, mp: KC.check_chunk_simple(d, B=1, H=2, T=21, Dk=64, Dv=128, dtype=BF16, with_h0=False), 4, 1),
    # short conv: x w mask cache, 2 step inputs, bias | y of 5 launches
    C("conv-f32", lambda d, mp: KC.check_conv(d, B=2, T=37, D=96, W=4, dtype=F32), 7, 5),
    C("conv-bf16", lambda d, mp: KC.check_conv(d, B=2, T=19, D=96, W=3, dtype=BF16), 7, 5),
    C("conv-one-token", lambda d, mp: KC.check_conv(d, B=2, T=1, D=96, W=4, dtype=F32), 5, 4),
    # conv backward: x w (bias) mask dy | y, dx, dw (partials)
    C("conv-bwd-f32", lambda d, mp: KC.check_conv_bwd(d, B=2, T=70, D=96, W=4, dtype=F32, use_bias=False, activation="silu"), 4, 3),
    C("conv-bwd-T5-bias", lambda d, mp: KC.check_conv_bwd(d, B=2, T=5, D=96, W=4, dtype=F32, use_bias=True, activation=None), 5, 3),
    C("conv-bwd-bf16", lambda d, mp: KC.check_conv_bwd(d, B=2, T=130, D=96, W=3, dtype=BF16, use_bias=True, activation="silu"), 5, 3),
    # fused q|k|v conv: z gk 3 w (3 b) mask do | the slab, 3 outputs
    C("conv3-f32", lambda d, mp: KC.check_short_conv3(d, 2, 70, 2, 64, F32, True, True), 10, 3),
    C("conv3-bf16", lambda d, mp: KC.check_short_conv3(d, 2, 70, 2, 64, BF16, True, False), 10, 3),
    # split_slab: z o cw nw dq do | slab, conv y, norm y
    C("split-slab-f32", lambda d, mp: KC.check_split_slab(d, 2, 70, 2, 64, F32, True), 6, 3),
    C("split-slab-bf16", lambda d, mp: KC.check_split_slab(d, 2, 70, 2, 64, BF16, True), 6, 3),
    # RMSNorm-gate: x gate w parts | y of four launches
    C("rmsnorm-f32", lambda d, mp: KC.check_rmsnorm(d, rows=7, D=64, dtype=F32), 4, 4),
    C("rmsnorm-bf16", lambda d, mp: KC.check_rmsnorm(d, rows=7, D=512, dtype=BF16), 4, 4),
    C("rmsnorm-bwd-f32", lambda d, mp: KC.check_rmsnorm_bwd(d, rows=9, D=256, dtype=F32, gate=True, affine=True), 4, 3),
    C("rmsnorm-bwd-bf16", lambda d, mp: KC.check_rmsnorm_bwd(d, rows=9, D=256, dtype=BF16, gate=True, affine=True), 4, 3),
    C("rmsnorm-bwd-no-gate", lambda d, mp: KC.check_rmsnorm_bwd(d, rows=9, D=64, dtype=F32, gate=False, affine=True), 3, 2),
    # K10: x (r) gamma beta wy ws | y (xs), dx
    C("k10-layer-norm-f32", lambda d, mp: KC.check_layer_norm(d, 13, 320, F32, F32, F32), 5, 2),
    C("k10-layer-norm-bf16", lambda d, mp: KC.check_layer_norm(d, 6, 128, BF16, BF16, BF16), 5, 2),
    C("k10-layer-norm-no-residual", lambda d, mp: KC.check_layer_norm(d, 9, 64, F32, None, F32), 4, 2),
    # K11: u w | y, du
    C("k11-swiglu-gate-odd-f32", lambda d, mp: KC.check_swiglu_gate(d, 7, 85, F32), 2, 2),
    C("k11-swiglu-gate-odd-bf16", lambda d, mp: KC.check_swiglu_gate(d, 3, 85, BF16), 2, 2),
    C("k11-swiglu-gate-vector", lambda d, mp: KC.check_swiglu_gate(d, 9, 128, BF16), 2, 2),
    # K12 / K12b: x w | y, dx  //  z w (b) dy | y, dlr, dW
    C("k12-gate-f32", lambda d, mp: KC.check_gate_logsigmoid(d, 4100, F32, -0.2), 2, 2),
    C("k12-gate-bf16", lambda d, mp: KC.check_gate_logsigmoid(d, 4100, BF16, None), 2, 2),
    C("k12b-lowrank-f32", lambda d, mp: KC.check_gate_lowrank(d, 2, 70, 64, 16, F32, None, True, True), 4, 3),
    C("k12b-lowrank-odd", lambda d, mp: KC.check_gate_lowrank(d, 2, 33, 64, 7, BF16, None, False, False), 3, 3),
    C("k12c-lowrank-aligned", lambda d, mp: KC.check_gate_lowrank(d, 2, 45, 320, 16, BF16, None, False, "aligned"), 3, 3),
    # channel mixer: x w_in b_in w_out b_out dy | y and the gradients
    C("swiglu-mlp-f32", lambda d, mp: KC.check_swiglu_mlp(d, 2, 70, 48, 21, F32, True), 6, 4),
    C("swiglu-mlp-bf16", lambda d, mp: KC.check_swiglu_mlp(d, 2, 70, 48, 21, BF16, True), 6, 4),
    # K14: logits targets (all-ignored targets) | loss, dlogits
    C("k14-cross-entropy-f32", lambda d, mp: KC.check_cross_entropy(d, 37, 131, F32, None), 2, 2),
    C("k14-cross-entropy-stride", lambda d, mp: KC.check_cross_entropy(d, 9, 64, BF16, 72), 2, 2),
    C("k14-cross-entropy-odd-width", lambda d, mp: KC.check_cross_entropy(d, 3, 5, BF16, 9), 2, 2),
    C("k14-cross-entropy-V1027", lambda d, mp: KC.check_cross_entropy(d, 20, 1027, F32, None), 2, 2),
    # K13 / K13a: 12 partial tensors | 12 sums (the width-3 case falls back to torch)  //  5 matrices, 3 vectors | sums (+ partials)
    C("k13-sum-partials", lambda d, mp: KC.check_sum_partials(d), 12, 12),
    C("k13a-column-sum", lambda d, mp: KC.check_column_sum(d), 8, 8),
    # K15 / K16: 4 weights | 3 padded operands  //  5 blocks x dy | the stacked operand (the products are torch GEMMs)
    C("k15-mlp-pack", lambda d, mp: (KC.check_mlp_pack(d), KC.check_mlp_pack(d, H=127, d_in=8, d_out=3)), 8, 6),
    C("k16-stacked-linear", lambda d, mp: KC.check_stacked_linear(d), 7, 1),
    # K17: 67 parameters and 3 rounds of gradients | 2 moments each
    C("k17-adamw", lambda d, mp: KC.check_fused_adamw(d), 67 * 4, 67 * 2),
    # embed / arg-max / sampler
    C("embed", lambda d, mp: KC.check_embed(d, Q=2, B=3, n=2, n_emb=37, d=64, dtype=F32), 2, 1),
    C("embed-bwd", lambda d, mp: KC.check_embed_bwd(d, Q=2, B=3, n=5, n_emb=11, d=64, dtype=F32), 3, 2),
    C("argmax-L4099", lambda d, mp: KC.check_argmax(d, rows=5, n=4099, dtype=F32), 2, 2),
    C("topk-n300-k7", lambda d, mp: KC.check_topk_sample(d, rows=6, n=300, k=7, temp=0.7, dtype=F32, draws=60), 5, 3),
    C("topk-n1030-bf16", lambda d, mp: KC.check_topk_sample(d, rows=6, n=1030, k=100, temp=0.9, dtype=BF16, draws=60), 5, 3),
    # K6d / K6e / K6f: table, log, step, counter (+ control block) and logits + x per step
    C("k6d-greedy-pick-embed", lambda d, mp: KC.check_greedy_pick_embed(d, B=5, Q=3, L=70, d=32, dtype=BF16), 4 + 2 * 5),
    C("k6d-loop-ctl", lambda d, mp: KC.check_pick_loop_ctl(d, B=5, Q=3, L=70, d=32, dtype=BF16, sampled=False), 4 + 2 * 6, 1),
    C("k6e-loop-ctl-sampled", lambda d, mp: KC.check_pick_loop_ctl(d, B=5, Q=2, L=70, d=32, dtype=F32, sampled=True), 4 + 2 * 6, 7),
    C("k6e-sample-pick-embed", lambda d, mp: KC.check_sample_pick_embed(d, B=5, Q=3, L=70, d=32, dtype=BF16, n_sampled=3), 4 + 3 * 4, 8),
    C("k6e-sample-pick-embed-f32", lambda d, mp: KC.check_sample_pick_embed(d, B=5, Q=2, L=50, d=20, dtype=F32, n_sampled=0), 4 + 2 * 4, 8),
    # table, forced tokens, 2 length arrays, 6 buffer sets of >= 4 and logits per step | control blocks, K6a outputs
    C("k6f-forced-B3-Q4", lambda d, mp: PC.check_pick_embed_forced(d, 3, 4, 64, BF16), 4 + 6 * 4 + 8, 4 + 8),
    C("k6f-forced-B1-Q1", lambda d, mp: PC.check_pick_embed_forced(d, 1, 1, 64, F32), 4 + 6 * 4 + 8, 4 + 8),
    C("k6f-forced-sampled", lambda d, mp: PC.check_pick_embed_forced(d, 3, 4, 64, BF16, ((True, True, False), (False, False, True)),
                                                                      n_sampled=1, k=10, temp=0.8, seed=11), 4 + 3 * 4 + 8, 2 + 8),
    # decode prologue: z, 3 filters, 3 caches, w2 b2, qkv, gk
    C("prologue-f32", lambda d, mp: KC.check_prologue(d, B=3, Kd=64, Vd=128, dtype=F32), 11),
    C("prologue-bf16", lambda d, mp: KC.check_prologue(d, B=2, Kd=64, Vd=64, dtype=BF16), 11),
    # decode_update: 5 operands, the cloned state, o_part | K1's o, S
    C("decode-update-f32", lambda d, mp: KC.check_decode_update(d, B=2, H=2, Dk=64, Dv=64, dtype=F32), 7, 2),
    C("decode-update-bf16", lambda d, mp: KC.check_decode_update(d, B=2, H=2, Dk=256, Dv=128, dtype=BF16), 7, 2),
    # with the fused norm: 5 operands, zrow, w, counters, 2 states + 3 buffers per repeat | the unfused norm's output
    C("decode-update-norm-f32", lambda d, mp: KC.check_decode_update_norm(d, B=2, H=2, Dk=64, Dv=64, dtype=F32, repeats=2), 10 + 6, 2),
    C("decode-update-norm-bf16", lambda d, mp: KC.check_decode_update_norm(d, B=2, H=2, Dk=256, Dv=128, dtype=BF16, repeats=2), 10 + 6, 2),
    # K1w: h0 w 2 counters 2 states 3 histories step origin (+ exchange) and q k v gk gate og per step
    C("k1w-f32-window8-partial", lambda d, mp: KC.check_decode_window(d, B=2, H=2, Dk=64, Dv=64, dtype=F32, window=8, n_steps=19), 11 + 6 * 19),
    C("k1w-bf16-window4", lambda d, mp: KC.check_decode_window(d, B=2, H=2, Dk=128, Dv=128, dtype=BF16, window=4, n_steps=9), 11 + 6 * 9),
    C("k1w-window1", lambda d, mp: KC.check_decode_window(d, B=2, H=2, Dk=64, Dv=64, dtype=F32, window=1, n_steps=3), 11 + 6 * 3),
    C("k1w-dv512-exchange", lambda d, mp: KC.check_decode_window(d, B=2, H=2, Dk=64, Dv=512, dtype=F32, window=4, n_steps=6), 12 + 6 * 6),
    C("k1w-dv512-bf16-window8", lambda d, mp: KC.check_decode_window(d, B=2, H=2, Dk=128, Dv=512, dtype=BF16, window=8, n_steps=9), 12 + 6 * 9),
    C("k1w-bf16-state-window1", lambda d, mp: KC.check_decode_window(d, B=2, H=2, Dk=256, Dv=256, dtype=BF16, window=1, n_steps=6,
                                                                     state_dtype=BF16), 10 + 6 * 6),
    C("k1w-bf16-state-dv512", lambda d, mp: KC.check_decode_window(d, B=2, H=2, Dk=64, Dv=512, dtype=BF16, window=4, n_steps=6,
                                                                   state_dtype=BF16), 11 + 6 * 6),
    # persistent K1w, grids 1, 3, 5 (below), 6 (= heads), 11 (above): 6 runs of (S 3 histories w origin + 7 tensors per step)
    C("k1w-persist-window8", lambda d, mp: check_persist_equals_plain(d, 2, 3, 64, 64, BF16, F32, 8, False), 6 * (6 + 7 * 17)),
    C("k1w-persist-window1-f32", lambda d, mp: check_persist_equals_plain(d, 2, 3, 64, 128, F32, F32, 1, False), 6 * (6 + 7 * 3)),
    C("k1w-persist-bf16-state", lambda d, mp: check_persist_equals_plain(d, 2, 3, 64, 256, BF16, BF16, 8, False, grids=(5, 6, 11)),
      4 * (6 + 7 * 17)),
    # skinny linear: a w (b) (r) (gamma beta) | out (the in-place residual form writes a clone)
    C("skinny-plain", lambda d, mp: KC.check_linear_skinny(d, M=5, N=20, K=64, dtype=F32), 2, 1),
    C("skinny-ln-swiglu", lambda d, mp: KC.check_linear_skinny(d, M=9, N=96, K=64, dtype=F32, ln=True, bias=True, swiglu=85), 5, 1),
    C("skinny-resid-M70", lambda d, mp: KC.check_linear_skinny(d, M=70, N=33, K=96, dtype=F32, resid=True, bias=True), 5, 1),
    C("skinny-bf16-ln", lambda d, mp: KC.check_linear_skinny(d, M=7, N=40, K=160, dtype=BF16, ln=True), 4, 1),
    C("skinny-bf16-resid-N17", lambda d, mp: KC.check_linear_skinny(d, M=3, N=17, K=352, dtype=BF16, resid=True), 4, 1),
    C("skinny-bf16-swiglu-M66", lambda d, mp: KC.check_linear_skinny(d, M=66, N=64, K=64, dtype=BF16, ln=True, bias=True, swiglu=37), 5, 1),
    # packed: a w (c1) c2 (r) out out_p out_p2 (rp) + the packed a and w | the row-major reference output
    C("skinny-packed-f32-resid", lambda d, mp: KC.check_linear_skinny_packed(d, 5, 40, 64, F32, ln=False, bias=True, resid=True, swiglu=0), 10, 1),
    C("skinny-packed-bf16-swiglu", lambda d, mp: KC.check_linear_skinny_packed(d, 7, 32, 64, BF16, ln=True, bias=True, resid=False, swiglu=21), 9, 1),
    C("skinny-packed-bf16-ln", lambda d, mp: KC.check_linear_skinny_packed(d, 20, 48, 64, BF16, ln=True, bias=True, resid=False, swiglu=0), 9, 1),
    C("skinny-8-waves", lambda d, mp: _wide_split_k(d, mp, 8), 9 + 20, 1),
    C("skinny-16-waves", lambda d, mp: _wide_split_k(d, mp, 16), 9 + 20, 1),
    # in-projection: x w gamma beta 3 filters 3 caches w2 b2, 6 cache clones, 5 outputs | z of the unfused projection
    C("inproj-f32", lambda d, mp: KC.check_inproj(d, B=5, K=64, Kd=32, Vd=48, dtype=F32), 23, 1),
    C("inproj-bf16-two-row-blocks", lambda d, mp: KC.check_inproj(d, B=70, K=64, Kd=64, Vd=32, dtype=BF16), 23, 1),
    # x w c2 5 weights 3 caches, 2 x (3 clones + 3 outputs), the packed x and w
    C("inproj-packed-f32", lambda d, mp: KC.check_inproj_packed(d, B=5, K=64, Kd=32, Vd=32, dtype=F32), 13 + 12),
    C("inproj-packed-bf16", lambda d, mp: KC.check_inproj_packed(d, B=5, K=64, Kd=32, Vd=32, dtype=BF16), 13 + 12),
    # tall linear (M not a multiple of 64): a w (c1 c2) (r) ref_sk out out_p (rp) + the packed a and w
    *[C(f"tall-v0-case{i}", _tall(i, 0), 7) for i in range(6)],
    *[C(f"tall-v{v}-case{i}", _tall(i, v), 7) for v in (1, 2) for i in (2, 4)],
    # tall in-projection: x w c2 5 weights 3 caches, the packed x and w, 2 (3 with same_as_variant) x (3 clones + 3 outputs)
    C("inproj-tall-v0-bf16", lambda d, mp: KC.check_inproj_tall(d, 130, 96, 64, 128, BF16, variant=0), 13 + 12),
    C("inproj-tall-v0-f32", lambda d, mp: KC.check_inproj_tall(d, 129, 48, 64, 64, F32, variant=0), 13 + 12),
    C("inproj-tall-v1", lambda d, mp: KC.check_inproj_tall(d, 70, 160, 128, 64, BF16, variant=1), 13 + 12),
    C("inproj-tall-v2", lambda d, mp: KC.check_inproj_tall(d, 129, 48, 64, 64, F32, variant=2), 13 + 12),
    C("inproj-tall-v3-bf16", lambda d, mp: KC.check_inproj_tall(d, 130, 256, 64, 128, BF16, variant=3, same_as_variant=0), 13 + 18),
    C("inproj-tall-v3-f32", lambda d, mp: KC.check_inproj_tall(d, 200, 128, 64, 64, F32, variant=3, same_as_variant=0), 13 + 18),
    # cross-attention step1/2: q kk vv pe ln_w ln_b x att xp xp2 x0
    C("cross-att-f32-Tn9", lambda d, mp: KC.check_cross_att(d, B=3, Tn=9, d=64, dtype=F32), 11),
    C("cross-att-bf16-Tn70", lambda d, mp: KC.check_cross_att(d, B=3, Tn=70, d=128, dtype=BF16), 11),
    # spread kernels: q kk vv ln_w ln_b scores att attc x x0
    C("cross-spread-f32-Tn9", lambda d, mp: KC.check_cross_spread(d, B=5, Tn=9, d=64, dtype=F32), 10),
    C("cross-spread-bf16-Tn70", lambda d, mp: KC.check_cross_spread(d, B=5, Tn=70, d=128, dtype=BF16), 10),
    # fusions: 5 operands, scores, 2 att, 2 attc, sc2, x0, x_a, x_b (+ the pe-scores and att-log forms at d % 256 == 0)
    C("cross-fused-f32-Tn11", lambda d, mp: KC.check_cross_fused(d, 3, 11, 64, F32), 14),
    C("cross-fused-bf16-Tn40", lambda d, mp: KC.check_cross_fused(d, 2, 40, 128, BF16), 14),
    C("cross-fused-f32-d256", lambda d, mp: KC.check_cross_fused(d, 2, 13, 256, F32), 14 + 8),
    C("cross-fused-bf16-d256", lambda d, mp: KC.check_cross_fused(d, 3, 33, 256, BF16), 14 + 8),
    # softmax_pe_rows with the attention log: scores pe att xp (xp_p) log step + (before, xp2) x 4
    C("softmax-pe-rows-f32", lambda d, mp: KC.check_softmax_pe_rows(d, 3, 11, 64, F32), 7 + 8),
    C("softmax-pe-rows-bf16-d256", lambda d, mp: KC.check_softmax_pe_rows(d, 3, 33, 256, BF16), 7 + 8),
    # ragged: 7 operands and per _launch (>= 6 of them) lengths, scores, att, xp, x
    C("cross-ragged-f32", lambda d, mp: _ragged(d, mp, 64, F32, False), 7 + 6 * 5),
    C("cross-ragged-bf16-d1024-shared-pe", lambda d, mp: _ragged(d, mp, 1024, BF16, True), 7 + 6 * 5),
    # vocoder: x w bias scale shift (x and w twice) | y, y2  //  frames window cut window | y, rec
    C("dwconv7-ln-f32", lambda d, mp: KC.check_dwconv7_ln(d, B=2, L=11, C=64, dtype=F32, ada=False), 7, 2),
    C("dwconv7-ln-bf16-ada", lambda d, mp: KC.check_dwconv7_ln(d, B=2, L=11, C=96, dtype=BF16, ada=True), 7, 2),
    C("istft-ola", lambda d, mp: KC.check_istft_ola(d, B=2, T=20, win=64, hop=16), 4, 2),
    C("istft-ola-T5", lambda d, mp: KC.check_istft_ola(d, B=2, T=5, win=40, hop=10), 4, 2),
]

# paths the emulator cannot exercise faithfully (LDS DMA, real wave scheduling between workgroups of one launch) or that take
# it too long; small shapes all the same
GPU_ONLY = [
    # the tall kernels with the LDS ring filled by DMA (variant 0), ragged M, N and K-stage counts
    C("tall-dma-ring-43-k-steps", lambda d, mp: KC.check_linear_tall(d, 130, 1024, 1376, BF16, resid=True, variant=0), 7),
    C("tall-dma-ring-f32-swiglu", lambda d, mp: KC.check_linear_tall(d, 129, 56, 288, F32, ln=True, bias=True, resid=True, swiglu=40,
                                                                     variant=0), 7),
    C("inproj-tall-dma-ring", lambda d, mp: KC.check_inproj_tall(d, 70, 160, 128, 64, BF16, variant=0), 13 + 12),
    # K2 of 256 x 512 heads as ONE launch of two workgroups per head (8 heads: the XCD-paired block-id mapping)
    C("k2-dv512-one-launch-8-heads", lambda d, mp: KC.check_chunk_dv512_one_launch(d, mp, B=1, H=8, T=33), 5, 6),
    C("k2-dv512-one-launch-3-heads", lambda d, mp: KC.check_chunk_dv512_one_launch(d, mp, B=1, H=3, T=36), 5, 6),
    # segment-parallel K2 / K2b at B > 1 with every batch row's own resets
    C("k2-segments-batch-rows", lambda d, mp: KC.check_chunk_segmented(d, B=3, H=2, T=100, nseg=4, resets="rows"), 5, 6),
    C("k2b-full-batch-rows", lambda d, mp: KC.check_chunk_bwd_full(d, 3, 2, 100, 256, 4, resets="rows", via_autograd=True), 7, 6),
    # the persistent K1w writing its output fragment-major
    C("k1w-persist-packed", lambda d, mp: check_persist_equals_plain(d, 2, 3, 256, 256, BF16, F32, 8, True), 6 * (6 + 7 * 17)),
    C("k1w-persist-packed-window1", lambda d, mp: check_persist_equals_plain(d, 2, 3, 64, 64, BF16, BF16, 1, True), 6 * (6 + 7 * 3)),
]


def _run(case, n_case, n_lib, dev, monkeypatch):
    failed = None
    with guarded(monkeypatch, dev) as arena:
        try:
            case(dev, monkeypatch)
        except AssertionError as e:          # a store past a row usually breaks parity too: report the bands as well
            failed = e
    if dev == "cuda":
        torch.cuda.synchronize()
    if failed is not None:
        try:
            arena.check()
        except GuardDamage as damage:
            raise GuardDamage(f"{damage}\nand the case's own assertion failed: {failed}") from failed
        raise failed
    n_own = arena.count - arena.count_launcher
    print(f"guarded tensors: {n_own} from the case, {arena.count_launcher} from the launchers")
    assert n_own >= n_case, f"only {n_own} tensors of the case function were guarded, expected at least {n_case}"
    assert arena.count_launcher >= n_lib, \
        f"only {arena.count_launcher} tensors allocated by the launchers were guarded, expected at least {n_lib}"
    arena.check()


@pytest.mark.parametrize("case,n_case,n_lib", CASES)
def test_guard_bands_emu(emu, monkeypatch, case, n_case, n_lib):
    _run(case, n_case, n_lib, "cpu", monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case,n_case,n_lib", CASES + GPU_ONLY)
def test_guard_bands_gpu(hip, monkeypatch, case, n_case, n_lib):
    _run(case, n_case, n_lib, "cuda", monkeypatch)
