"""Shared checks of the ragged vocoder: codes of different lengths to waveforms in one batch.  Row b of a
right-padded batch must be what that row's own positions give ALONE -- the same operator or module on ``[..., :L_b]`` of the
row as a batch of one:
  * K8r ``dwconv7_ln_ragged``, K9r ``istft_ola_ragged``, K10g ``group_norm_ragged``: against the fp64 oracle
    (``oracle.vocoder_oracle``, ``F.group_norm``) on the row alone at the tolerances of the uniform kernels' checks, exact
    zeros past the row's end, BIT-equal to the uniform entry on the row alone, and bit-identical when the padding is NaN;
  * ``WavTokenizerDecoder(..., lens=...)`` against ``OracleVocoder`` and against the product's own alone call;
  * ``LinaModel.synthesize`` against ``generate_queue`` + one vocoder call per utterance.
The kernel cases put their operands on ``dev`` with the one-argument ``.to(dev)`` (tests/guard.py routes those, and the outputs
the launchers allocate, into a guard arena); the ``*_N_CASE`` / ``*_N_LIB`` constants are the numbers of such tensors, read off
each case.
`dev` = "cpu" (ops bound to the wave64 emulator) or "cuda"."""
import pytest
import torch
import torch.nn.functional as F

import queue_cases as QC
from kernel_cases import assert_close
from lina_speech_amd import ops
from lina_speech_amd.vocoder import WavTokenizerDecoder
from oracle import vocoder_oracle as VO

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _tol(dtype):
    return 1e-5 if dtype == F32 else 2e-2           # K8's own tolerances (kernel_cases.check_dwconv7_ln)


def _nan_pads(x, lens, dim):
    """A copy of ``x`` whose positions >= lens[b] along ``dim`` of row b hold NaN."""
    x = x.clone()
    for b, L in enumerate(lens):
        x[b].narrow(dim - 1, L, x.shape[dim] - L).fill_(float("nan"))
    return x


# ----------------------------------------------------------------------------- K8r
K8R_B, K8R_L, K8R_LENS = 5, 11, [1, 7, 8, 9, 11]        # one row, one below / at / one above K8's 8-row run, full
K8R_CASES = [(64, F32, False), (96, BF16, True)]
# operands x w bias scale shift lens + the NaN-padded x + one alone x per row | y, y (NaN pads), one alone y per row
K8R_N_CASE, K8R_N_LIB = 6 + 1 + K8R_B, 2 + K8R_B


def check_dwconv7_ln_ragged(dev, C, dtype, ada):
    B, L, lens = K8R_B, K8R_L, K8R_LENS
    g = torch.Generator().manual_seed(131)
    x = torch.randn(B, L, C, generator=g).to(dtype)
    w = (torch.randn(C, 1, 7, generator=g) * 0.4).to(dtype)
    bias = torch.randn(C, generator=g).to(dtype)
    scale = (1 + 0.3 * torch.randn((B, C) if ada else (C,), generator=g)).to(dtype)
    shift = (0.3 * torch.randn((B, C) if ada else (C,), generator=g)).to(dtype)
    xd, wd, bd, sd, hd = x.to(dev), w.to(dev), bias.to(dev), scale.to(dev), shift.to(dev)
    ld = torch.tensor(lens, dtype=torch.int32).to(dev)
    y = ops.dwconv7_ln_ragged(xd, wd, bd, sd, hd, 1e-6, lens=ld)
    assert y.dtype == dtype and y.shape == x.shape
    y_nan = ops.dwconv7_ln_ragged(_nan_pads(x, lens, 1).to(dev), wd, bd, sd, hd, 1e-6, lens=ld)
    assert same_bits(y, y_nan), "K8r: NaN past a row's end changed the output"
    for b, Lb in enumerate(lens):
        row = lambda t: t[b:b + 1] if ada else t
        ref = VO.dwconv7_ln(x[b:b + 1, :Lb].to(F64), w.to(F64), bias.to(F64), row(scale).to(F64), row(shift).to(F64), 1e-6)
        assert_close(y[b:b + 1, :Lb], ref, _tol(dtype), f"K8r row {b} (L = {Lb}) vs the oracle on the row alone")
        assert bool((y[b, Lb:] == 0).all()), f"K8r row {b}: not zero past its end"
        alone = ops.dwconv7_ln(x[b:b + 1, :Lb].contiguous().to(dev), wd, bd, row(sd), row(hd), 1e-6)
        assert same_bits(y[b:b + 1, :Lb], alone), f"K8r row {b} (L = {Lb}) is not bit-equal to K8 on the row alone"


# ----------------------------------------------------------------------------- K9r
K9R_CASES = [((4, 6, 40, 10), [1, 2, 5, 6]), ((4, 20, 64, 16), [1, 4, 19, 20])]     # T_b = 1 and T_b < win / hop: the gather's edges
# frames window lens + NaN-padded frames + one alone frames per row | y, y (NaN pads), one alone y per row
K9R_N_CASE, K9R_N_LIB = 3 + 1 + 4, 2 + 4


def check_istft_ola_ragged(dev, shape, lens):
    B, T, win, hop = shape
    g = torch.Generator().manual_seed(132)
    frames = torch.randn(B, T, win, generator=g)
    window = torch.hann_window(win)
    fd, wd = frames.to(dev), window.to(dev)
    ld = torch.tensor(lens, dtype=torch.int32).to(dev)
    y = ops.istft_ola_ragged(fd, wd, hop, ld)
    assert y.shape == (B, T * hop) and y.dtype == F32
    y_nan = ops.istft_ola_ragged(_nan_pads(frames, lens, 1).to(dev), wd, hop, ld)
    assert same_bits(y, y_nan), "K9r: NaN in the frames past a row's end changed the output"
    for b, Tb in enumerate(lens):
        ref = VO.istft_same(frames[b:b + 1, :Tb].to(F64), window.to(F64), hop)
        assert_close(y[b:b + 1, :Tb * hop], ref, 1e-5, f"K9r row {b} (T = {Tb}) vs the oracle on the row alone")
        assert bool((y[b, Tb * hop:] == 0).all()), f"K9r row {b}: not zero past its end"
        alone = ops.istft_ola(frames[b:b + 1, :Tb].contiguous().to(dev), wd, hop)
        assert same_bits(y[b:b + 1, :Tb * hop], alone), f"K9r row {b} (T = {Tb}) is not bit-equal to K9 on the row alone"


# ----------------------------------------------------------------------------- K10g
# (B, C, G, Lmax), lens, dtype; the last: 24 x 300 = 7200 elements per group, several passes of the 256-thread workgroup
K10G_CASES = [((4, 64, 32, 11), [1, 2, 7, 11], F32), ((4, 96, 32, 11), [1, 2, 7, 11], BF16), ((2, 768, 32, 300), [37, 300], F32)]


def k10g_counts(B):
    # x weight bias lens + one alone x per row + permuted x and lens + NaN-padded x | y, y (lens=None), alone y per row, permuted, NaN
    return 4 + B + 2 + 1, 2 + B + 1 + 1


def check_group_norm_ragged(dev, shape, lens, dtype, act):
    B, C, G, L = shape
    eps = 1e-6
    g = torch.Generator().manual_seed(133)
    x = (torch.randn(B, C, L, generator=g) * 1.5 + 0.5 * torch.randn(B, C, 1, generator=g)).to(dtype)
    weight = (1 + 0.3 * torch.randn(C, generator=g)).to(dtype)
    bias = (0.3 * torch.randn(C, generator=g)).to(dtype)

    def ref(xs):
        r = F.group_norm(xs.to(F64), G, weight.to(F64), bias.to(F64), eps)
        return F.silu(r) if act == "silu" else r

    xd, wd, bd = x.to(dev), weight.to(dev), bias.to(dev)
    ld = torch.tensor(lens, dtype=torch.int32).to(dev)
    y = ops.group_norm_ragged(xd, G, wd, bd, eps, act, ld)
    assert y.dtype == dtype and y.shape == x.shape
    full = ops.group_norm_ragged(xd, G, wd, bd, eps, act, None)
    assert_close(full, ref(x), _tol(dtype), f"K10g lens=None vs F.group_norm ({act})")
    for b, Lb in enumerate(lens):
        assert_close(y[b:b + 1, :, :Lb], ref(x[b:b + 1, :, :Lb]), _tol(dtype),
                     f"K10g row {b} (L = {Lb}, {act}) vs F.group_norm on the row alone")
        assert bool((y[b, :, Lb:] == 0).all()), f"K10g row {b}: not zero past its end"
        alone = ops.group_norm_ragged(x[b:b + 1, :, :Lb].contiguous().to(dev), G, wd, bd, eps, act, None)
        assert same_bits(y[b:b + 1, :, :Lb], alone), \
            f"K10g row {b} (L = {Lb}) is not bit-equal to the row alone (another Lmax and row stride)"
    perm = list(reversed(range(B)))
    y_p = ops.group_norm_ragged(x[perm].contiguous().to(dev), G, wd, bd, eps, act,
                                torch.tensor([lens[i] for i in perm], dtype=torch.int32).to(dev))
    assert same_bits(y_p, y[perm]), "K10g: permuting the rows changed a row's bits"
    y_nan = ops.group_norm_ragged(_nan_pads(x, lens, 2).to(dev), G, wd, bd, eps, act, ld)
    assert same_bits(y, y_nan), "K10g: NaN past a row's end changed the output"


def check_kernel_argument_errors(dev):
    """Bad arguments are refused by the launchers or come back as LINA_ERR_ARG: nothing is launched."""
    x = torch.randn(2, 6, 64).to(dev)
    w = torch.randn(64, 7).to(dev)
    good = torch.tensor([3, 6], dtype=torch.int32).to(dev)
    with pytest.raises(TypeError):
        ops.dwconv7_ln_ragged(x, w, lens=torch.tensor([3, 6]).to(dev))              # int64
    with pytest.raises(TypeError):
        ops.dwconv7_ln_ragged(x, w, lens=good[:1])
    with pytest.raises(TypeError):
        ops.istft_ola_ragged(x, torch.hann_window(64).to(dev), 16, None)
    with pytest.raises(ValueError):
        ops.istft_ola_ragged(x, torch.hann_window(64).to(dev), 15, good)            # win - hop odd
    with pytest.raises(ValueError):
        ops.group_norm_ragged(x, 4, lens=good)                                      # C = 6 channels, 4 groups
    with pytest.raises(ValueError):
        ops.group_norm_ragged(x, 3, act="gelu")
    lib = ops.get_backend().lib
    import ctypes
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    z = ctypes.c_void_p(0)
    assert lib.lina_dwconv7_ln_ragged(p(x), p(w), z, z, z, p(x), z, 2, 6, 64, 0, 1e-6, 0, z) == -1
    assert b"null" in lib.lina_last_error()
    assert lib.lina_group_norm_ragged(p(x), z, z, p(x), z, 2, 6, 64, 4, 1e-6, 0, 0, z) == -1
    assert b"divisible" in lib.lina_last_error()
    assert lib.lina_group_norm_ragged(p(x), z, z, p(x), z, 2, 6, 64, 3, 1e-6, 7, 0, z) == -1
    assert b"act" in lib.lina_last_error()


# ----------------------------------------------------------------------------- the module
SMALL = dict(codebook_dim=32, dim=64, intermediate_dim=128, num_layers=2, adanorm_num_embeddings=4, n_fft=64, hop_length=16)
MOD_LENS = [1, 7, 8, 9, 23]
MOD_L = 23
HOP = SMALL["hop_length"]

_SHARED = {}


def perturb(voc):
    """As test_full_size_vocoder_matches_cpu_oracle perturbs the weights: layer scales and AdaLayerNorm rows off their
    initial values, a head whose magnitudes stay below the clamp."""
    with torch.no_grad():
        for name, p in voc.named_parameters():
            if "gamma" in name or "scale" in name or "shift" in name:
                p.add_(torch.randn_like(p) * 0.1)
        voc.head.out.weight.mul_(0.2)
    return voc


def small_vocoder(n_codes=50, seed=10):
    torch.manual_seed(seed)
    return perturb(WavTokenizerDecoder(n_codes=n_codes, **SMALL).eval())


def module_case(dev):
    """(vocoder on dev, its CPU state dict, codes [1,5,23], bandwidth id, the ragged call's output, the alone calls' outputs):
    computed once per device and shared, never modified."""
    if dev not in _SHARED:
        voc = small_vocoder()
        sd = {k: v.detach().clone() for k, v in voc.state_dict().items()}
        g = torch.Generator().manual_seed(10)
        codes = torch.randint(0, 50, (1, len(MOD_LENS), MOD_L), generator=g)
        bw = torch.tensor([0])
        voc = voc.to(dev)
        audio = voc(codes.to(dev), bandwidth_id=bw.to(dev), lens=MOD_LENS)
        alone = [voc(codes[:, b:b + 1, :L].to(dev), bandwidth_id=bw.to(dev)) for b, L in enumerate(MOD_LENS)]
        _SHARED[dev] = (voc, sd, codes, bw, audio, alone)
    return _SHARED[dev]


def _rel(got, ref):
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all())
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def check_module_rows(dev):
    """Every row of the ragged call against the fp64 oracle on the row alone (5e-4 of the row's max, the bound of the uniform
    vocoder tests) and against the product's own call on the row alone (1e-5: the library convolutions may pick an algorithm
    by shape, so not bit-exact); exact zeros past the row's end.

    The second check uses an fp32 result as its reference at 1e-5, so the reference itself must be that good: the alone call
    is first held against the oracle at the same 1e-5 (no new code runs in it).  This is a condition on the INPUT: with
    dim = 64 a group holds two channels, and in the row of one frame a GroupNorm normalises two numbers, d / sqrt(d^2 + eps)
    with d half their difference -- a gain of up to eps^-1/2 = 1000 on the rounding errors of whatever came before when the
    two nearly coincide.  (Weights of seed 3 with codes of seed 134 hold such a pair, 0.005 apart: there the uniform path
    itself is 1.3e-4 from the oracle, the ragged call 6e-5, and the two 1.9e-4 from each other; eight other seeds in a row
    gave 3e-7 .. 5e-6 for every row.)"""
    voc, sd, codes, bw, audio, alone = module_case(dev)
    assert audio.shape == (len(MOD_LENS), MOD_L * HOP) and audio.dtype == F32
    orc = VO.OracleVocoder(sd, SMALL["num_layers"], SMALL["n_fft"], HOP)
    for b, L in enumerate(MOD_LENS):
        feats = sd["codebook"][0][codes[0, b:b + 1, :L]].transpose(1, 2)
        ref = orc.decode(feats, bw)
        e_orc = _rel(audio[b:b + 1, :L * HOP], ref)
        e_own = _rel(audio[b:b + 1, :L * HOP], alone[b])
        e_ref = _rel(alone[b], ref)
        print(f"ragged vocoder row {b} (L = {L}): vs oracle {e_orc:.2e}, vs the alone call {e_own:.2e} (alone call vs oracle "
              f"{e_ref:.2e})")
        assert e_ref < 1e-5, f"row {b}: the alone call is {e_ref:.2e} from the oracle -- no reference at 1e-5 (ill-conditioned input)"
        assert e_orc < 5e-4, f"row {b} (L = {L}): {e_orc:.2e} from the oracle on the row alone"
        assert e_own < 1e-5, f"row {b} (L = {L}): {e_own:.2e} from the product's own alone call"
        assert bool((audio[b, L * HOP:] == 0).all()), f"row {b}: not zero past its end"


def check_module_pads_uniform_list(dev):
    """Other valid ids as pad codes: bit-identical; all lengths Lmax: bit-identical to the uniform call; the list form: the
    same rows trimmed."""
    voc, sd, codes, bw, audio, alone = module_case(dev)
    g = torch.Generator().manual_seed(135)
    other = codes.clone()
    for b, L in enumerate(MOD_LENS):
        other[:, b, L:] = torch.randint(0, 50, (1, MOD_L - L), generator=g)
    assert not torch.equal(other, codes)
    assert same_bits(voc(other.to(dev), bandwidth_id=bw.to(dev), lens=MOD_LENS), audio), "the pad codes reached the output"
    uniform = voc(codes.to(dev), bandwidth_id=bw.to(dev))
    assert same_bits(voc(codes.to(dev), bandwidth_id=bw.to(dev), lens=[MOD_L] * len(MOD_LENS)), uniform)
    rows = voc([other[:, b, :L].to(dev) for b, L in enumerate(MOD_LENS)], bandwidth_id=bw.to(dev))
    assert isinstance(rows, list) and len(rows) == len(MOD_LENS)
    for b, L in enumerate(MOD_LENS):
        assert rows[b].shape == (L * HOP,) and same_bits(rows[b], audio[b, :L * HOP]), f"list form, row {b}"
    # codes_to_features zeroes past the row's end (lens as a LongTensor)
    feats = voc.codes_to_features(codes.to(dev), lens=torch.tensor(MOD_LENS))
    assert bool((feats[0, :, 1:] == 0).all()) and bool((feats[1, :, 7:] == 0).all()) and bool((feats[1, :, :7] != 0).any())


def check_module_errors(dev):
    voc, sd, codes, bw, audio, alone = module_case(dev)
    c = codes.to(dev)
    for bad in ([1, 7, 8, 9], [1, 7, 8, 9, 23, 23], [0, 7, 8, 9, 23], [1, 7, 8, 9, 24], torch.tensor([[1, 7, 8, 9, 23]]),
                [1.5, 7, 8, 9, 23]):
        with pytest.raises(ValueError):
            voc(c, bandwidth_id=bw.to(dev), lens=bad)
    with pytest.raises(ValueError):
        voc.decode(voc.codes_to_features(c), bw.to(dev), lens=[0, 7, 8, 9, 23])
    with pytest.raises(ValueError):
        voc([c[:, b, :L] for b, L in enumerate(MOD_LENS)], bandwidth_id=bw.to(dev), lens=MOD_LENS)


def check_full_size_row(dev):
    """The WavTokenizer-sized decoder (dim 768, 12 ConvNeXt blocks, n_fft 1280, hop 320), fp32, codes [1,3,60] with
    lens [1,33,60]: the row of 33 frames against the fp64 oracle on that row alone, 5e-4 of its max; zeros past every end."""
    torch.manual_seed(3)
    voc = perturb(WavTokenizerDecoder().eval())
    lens = [1, 33, 60]
    codes = torch.randint(0, 4096, (1, 3, 60))
    bw = torch.tensor([0])
    sd = {k: v.detach().clone() for k, v in voc.state_dict().items()}
    b, L = 1, 33
    feats = sd["codebook"][0][codes[0, b:b + 1, :L]].transpose(1, 2)
    ref = VO.OracleVocoder(sd, 12, 1280, 320).decode(feats, bw)
    voc = voc.to(dev)
    audio = voc(codes.to(dev), bandwidth_id=bw.to(dev), lens=lens)
    assert audio.shape == (3, 60 * 320)
    err = _rel(audio[b:b + 1, :L * 320], ref)
    print(f"full-size ragged vocoder, row of {L} frames vs oracle: {err:.2e}")
    assert err < 5e-4, err
    for i, Li in enumerate(lens):
        assert bool((audio[i, Li * 320:] == 0).all()) and bool(torch.isfinite(audio[i]).all())


# ----------------------------------------------------------------------------- synthesize
# the small queue model with peaked logits never stops: an utterance's cut grows with its step cap, and a cap of 1 leaves an
# empty cut (utterances 1 and 5); small caps keep the emulated decode short
SYN_CAPS = (3, 1, 5, 2, 4, 1, 6, 2, 3, 5)
SYN_KW = dict(max_seqlen=list(SYN_CAPS), stop_check_every=8)


def synth_case(dev):
    """(model, texts, vocoder, bandwidth id, generate_queue's codes, synthesize's waveforms at batch_size 3 / vocoder_batch 2):
    once per device, shared, never modified."""
    import ragged_cases as RC
    key = ("synth", dev)
    if key not in _SHARED:
        model = RC.tiny_model(dev)
        texts = [t.to(dev) for t in QC.queue_texts()]
        voc = small_vocoder(n_codes=model.n_codebook, seed=11).to(dev)
        codes = [c for c, _ in model.generate_queue(texts, batch_size=3, device=dev, **SYN_KW, **QC.GREEDY)]
        bw = torch.tensor([0]).to(dev)
        wavs = model.synthesize(texts, voc, 3, vocoder_batch=2, bandwidth_id=bw, device=dev, **SYN_KW, **QC.GREEDY)
        _SHARED[key] = (model, texts, voc, bw, codes, wavs)
    return _SHARED[key]


def check_synthesize_equals_alone(dev):
    """Waveform i has len(codes_i) * hop samples and equals the vocoder on codes_i alone (1e-5 of its max), codes_i from
    generate_queue with the same arguments; an utterance whose cut is empty (step cap 1) gives an empty tensor at its place."""
    model, texts, voc, bw, codes, wavs = synth_case(dev)
    assert len(wavs) == len(texts)
    lengths = [int(c.shape[-1]) for c in codes]
    assert lengths.count(0) >= 1 and len(set(lengths)) >= 4, f"the cuts must differ in length and one must be empty: {lengths}"
    for i, (c, wav) in enumerate(zip(codes, wavs)):
        assert wav.dim() == 1 and wav.dtype == F32 and wav.shape[0] == c.shape[-1] * HOP, \
            f"utterance {i}: {tuple(wav.shape)} for {c.shape[-1]} codes"
        if c.shape[-1] == 0:
            continue
        err = _rel(wav[None], voc(c.to(dev), bandwidth_id=bw))
        print(f"synthesize: utterance {i} ({c.shape[-1]} codes): {err:.2e} from the vocoder on its codes alone")
        assert err < 1e-5, f"utterance {i}: {err:.2e}"


def check_synthesize_vocoder_batch(dev):
    """vocoder_batch = 1 and N against 2: the same waveforms within 1e-5 of each one's max.  The groups are formed by
    ``LinaModel.vocode``, the half of ``synthesize`` behind the decode: it is called on generate_queue's codes, so that the
    queue is not decoded again for every group size (on the emulator a queue decode takes a minute)."""
    model, texts, voc, bw, codes, wavs = synth_case(dev)
    for vb in (1, len(texts)):
        got = model.vocode(codes, voc, vocoder_batch=vb, bandwidth_id=bw)
        assert len(got) == len(wavs)
        for i, (a, b) in enumerate(zip(got, wavs)):
            assert a.shape == b.shape
            if a.numel():
                err = _rel(a[None], b[None])
                assert err < 1e-5, f"vocoder_batch = {vb}, utterance {i}: {err:.2e}"


def check_synthesize_errors(dev):
    """A vocoder with fewer codes than the model emits raises, and so do generate_stream's own restrictions; an empty queue
    gives an empty list."""
    model, texts, voc, bw, codes, wavs = synth_case(dev)
    assert model.synthesize([], voc, 3, device=dev, **QC.GREEDY) == []
    small = small_vocoder(n_codes=model.n_codebook - 1).to(dev)
    with pytest.raises(ValueError):
        model.synthesize(texts[:2], small, 2, device=dev, max_seqlen=4, **QC.GREEDY)
    with pytest.raises(NotImplementedError):
        model.synthesize(texts[:2], voc, 2, device=dev, max_seqlen=4, prompt=torch.ones(1, 1, 2, dtype=torch.long), **QC.GREEDY)
    with pytest.raises(ValueError):
        model.synthesize(texts[:2], voc, 2, vocoder_batch=0, device=dev, max_seqlen=4, **QC.GREEDY)


# ----------------------------------------------------------------------------- guard bands
def run_guarded(case, n_case, n_lib, dev, monkeypatch):
    """``case()`` with its operands and the launchers' outputs between NaN-filled guard bands (tests/guard.py): its own
    assertions, at least ``n_case`` / ``n_lib`` guarded tensors from the case / the launchers, every band intact."""
    from guard import guarded
    with guarded(monkeypatch, dev) as arena:
        case()
    if dev == "cuda":
        torch.cuda.synchronize()
    n_own = arena.count - arena.count_launcher
    print(f"guarded tensors: {n_own} from the case, {arena.count_launcher} from the launchers")
    assert n_own >= n_case, f"only {n_own} tensors of the case function were guarded, expected at least {n_case}"
    assert arena.count_launcher >= n_lib, \
        f"only {arena.count_launcher} tensors allocated by the launchers were guarded, expected at least {n_lib}"
    arena.check()
