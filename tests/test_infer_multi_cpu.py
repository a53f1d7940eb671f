"""Several expressions per image (InferenceRunner.segment / InferEngine.forward_multi) without a GPU: every library launch is
replaced by a recorder (host logic only).  The visual encoder and the image-side neck convolutions must run at the IMAGE batch,
everything that reads the sentence at the EXPRESSION batch, and the schedule must be the image stage of a batch-B forward plus
the expression stage of a batch-K forward plus three gathers.  The numerics are tested on the GPU (tests/test_infer_multi_gpu.py)."""
import collections
import dataclasses

import pytest
import torch

from cris.pytorch_amd import arch, hip, ops, synth
from cris.pytorch_amd.engine import Engine
from cris.pytorch_amd.infer import InferenceRunner

IMAGE_SIDE = ("backbone.visual.", "neck.f1_v_proj.", "neck.f2_v_proj.", "neck.f3_v_proj.")


class _Stream:
    cuda_stream = 0

    def wait_stream(self, other):
        pass


@pytest.fixture
def recorder(monkeypatch):
    log = []
    monkeypatch.setattr(hip, "call", lambda name, *args: log.append((name, args)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _Stream())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert ops.hip is hip
    return log


@pytest.fixture
def stage_counter(monkeypatch, recorder):
    """launches issued inside the image-side parts of a schedule: _encode_image, the f2 / f3_v_proj conv+BN(+pool) layers and
    _fpn_image (forward_multi)"""
    counts = collections.Counter()

    def wrap(cls, meth, tag=None):
        inner = getattr(cls, meth)

        def f(self, *a, **k):
            n0 = len(recorder)
            out = inner(self, *a, **k)
            name = tag(a) if tag is not None else meth
            if name:
                counts[name] += len(recorder) - n0
            return out
        monkeypatch.setattr(cls, meth, f)

    from cris.pytorch_amd import infer
    wrap(Engine, "_encode_image")
    wrap(infer.InferEngine, "_fpn_image")
    wrap(Engine, "conv_bn", tag=lambda a: "neck_v_proj" if a[1] in ("neck.f2_v_proj.0", "neck.f3_v_proj.0") else None)
    return counts


def _weight_names(e):
    """[(first byte, end byte, parameter name)] of every GEMM weight operand the engine can launch with"""
    spans = [(t, name) for name, t in e.WF.items()]
    spans += [(v[0], wname) for (wname, _), v in e._fold.items()]
    return [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name) for t, name in spans]


def _gemms(log, e):
    """(weight name, M) of every GEMM launch of a recorded schedule, grouped launches unrolled"""
    spans = _weight_names(e)

    def name(ptr):
        hit = [n for a, b, n in spans if a <= ptr < b]
        assert len(hit) == 1, (ptr, hit)
        return hit[0]
    out = []
    for n, args in log:
        if n == "cris_conv_gemm_variant":
            probs = [args[0]._obj]
        elif n == "cris_conv_gemm_group_launch":
            g = args[0]._obj
            probs = [g.prob[i] for i in range(g.n)]
        else:
            continue
        out += [(name(p.Wt), p.M) for p in probs]
    return out


def _image_side(name):
    return name.startswith(IMAGE_SIDE)


@pytest.mark.parametrize("spec,size,word_len", [("tiny", 96, 9), ("r50", 416, 17)])
@pytest.mark.parametrize("fold", [True, False])
def test_multi_schedule(recorder, stage_counter, spec, size, word_len, fold):
    B, K = 2, 5
    index = [1, 0, 1, 1, 0]                         # not monotone, repeats
    clip, head = arch.specs_by_name(spec)
    head = dataclasses.replace(head, word_len=word_len)
    sd = arch.synthetic_state_dict(clip, head, 0)
    img, _, _ = synth.make_batch(B, size, word_len, 0, 0)
    imgK, word, _ = synth.make_batch(K, size, word_len, 0, 1)
    r = InferenceRunner(clip, head, sd, torch.device("cpu"), fold_bn=fold, use_graph=False)
    e = r.engine

    def record(fn):
        fn()                                        # first call: folds, packs, sizes the zero slab
        del recorder[:]
        stage_counter.clear()
        out = fn()
        return list(recorder), dict(stage_counter), out

    logB, cntB, _ = record(lambda: r(img, word[:B]))
    logK, cntK, _ = record(lambda: r(imgK, word))
    logM, cntM, out = record(lambda: r.segment(img, word, index))
    assert tuple(out.shape) == (K, 1, size // 4, size // 4)

    gathers = [a for n, a in logM if n == "cris_gather_samples_bf16"]
    assert len(gathers) == 3
    for a in gathers:
        assert a[4] == K                            # K rows of samples out
    # image stage: the visual encoder + f1_v_proj's convolution + f2 / f3_v_proj's conv+BN(+pool), at batch B
    img_runner = lambda c: c["_encode_image"] + c["neck_v_proj"] + 1          # noqa: E731  (+1: the f1_v_proj convolution)
    assert cntM["_encode_image"] + cntM["_fpn_image"] == img_runner(cntB)
    # (the count is not batch-free: a tile variant chosen for a larger M can bring a launch of its own)
    # the whole schedule: image stage at B + expression stage at K + the three gathers
    assert len(logM) == img_runner(cntB) + (len(logK) - img_runner(cntK)) + 3
    gB, gK, gM = _gemms(logB, e), _gemms(logK, e), _gemms(logM, e)
    mB = collections.defaultdict(list)
    mK = collections.defaultdict(list)
    for n, m in gB:
        mB[n].append(m)
    for n, m in gK:
        mK[n].append(m)
    seen = collections.defaultdict(int)
    n_img = n_expr = 0
    for n, m in gM:
        i = seen[n]
        seen[n] += 1
        if _image_side(n):
            assert m == mB[n][i] and m % B == 0 and m != mK[n][i], (n, m)
            n_img += 1
        else:
            assert m == mK[n][i], (n, m)
            n_expr += 1
    assert n_img == sum(1 for n, _ in gB if _image_side(n))
    assert n_expr == sum(1 for n, _ in gK if not _image_side(n))
    # the image-side GEMMs' M really is per image: B * OH * OW
    for n, args in logM:
        if n == "cris_conv_gemm_variant":
            p = args[0]._obj
            if _image_side(_gemms([(n, args)], e)[0][0]) and p.OH > 1:
                assert p.M == B * p.OH * p.OW


def _runner_for(spec, size, word_len):
    clip, head = arch.specs_by_name(spec)
    head = dataclasses.replace(head, word_len=word_len)
    return clip, head, arch.synthetic_state_dict(clip, head, 0)


@pytest.mark.parametrize("bad,msg", [
    ([], "K = 0"),
    ([0, 1], "2 image indices for 3 expressions"),
    ([0, 2, 1], "out of range"),
    ([0, -1, 1], "out of range"),
    ([0, 1.0, 1], "integers"),
])
def test_index_validation(recorder, bad, msg):
    clip, head, sd = _runner_for("tiny", 96, 9)
    r = InferenceRunner(clip, head, sd, torch.device("cpu"), use_graph=False)
    img, word, _ = synth.make_batch(2, 96, 9, 0, 0)
    word3 = torch.cat([word, word[:1]])
    if msg == "K = 0":
        word3 = word3[:0]
    with pytest.raises(ValueError, match=msg):
        r.segment(img, word3, bad)
    assert not recorder                              # nothing was launched
    with pytest.raises(ValueError, match="out of range"):
        r.segment(img, word3[:2] if msg != "K = 0" else word[:2], torch.tensor([0, 2]))
    with pytest.raises(ValueError, match="1-d integer"):
        r.segment(img, word[:2], torch.tensor([0.0, 1.0]))


def test_device_index_rejected(recorder):
    clip, head, sd = _runner_for("tiny", 96, 9)
    r = InferenceRunner(clip, head, sd, torch.device("cpu"), use_graph=False)
    img, word, _ = synth.make_batch(2, 96, 9, 0, 0)
    idx = torch.tensor([0, 1]).to("meta")            # any non-CPU tensor: checking its values would need a synchronisation
    with pytest.raises(ValueError, match="host sequence or a CPU tensor"):
        r.segment(img, word, idx)
    assert not recorder
