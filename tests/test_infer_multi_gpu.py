"""Several expressions per image with one visual pass (InferenceRunner.segment, CRIS.segment_expressions) on the GPU: the
image stage at batch B, the expression stage at batch K, joined by exact per-sample gathers (csrc/elementwise.hip
cris_gather_samples_bf16).  Against the batch forward of the same runner (bit for bit where the launches are the same), against
itself under permutations, against the CPU oracle, and graph replay against eager launches."""
import dataclasses
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import arch, evalpost, synth  # noqa: E402
from cris.pytorch_amd.infer import InferenceRunner  # noqa: E402
from oracle import cris_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _setup(spec, size, word_len):
    clip, head = arch.specs_by_name(spec)
    head = dataclasses.replace(head, word_len=word_len)
    return clip, head, arch.synthetic_state_dict(clip, head, 0)


def _inputs(B, K, size, word_len, step=0):
    img, _, _ = synth.make_batch(B, size, word_len, 0, step)
    _, word, _ = synth.make_batch(K, size, word_len, 0, step + 100)
    return img.to(DEV), word.to(DEV)


@pytest.mark.parametrize("spec,B,size,word_len", [("tiny", 3, 96, 9), ("r50", 2, 416, 17)])
@pytest.mark.parametrize("fold", [True, False])
def test_identity_index_equals_batch_forward(spec, B, size, word_len, fold):
    """B == K, index = arange(K): the image stage runs the batch forward's launches at the same M and the gathers copy rows"""
    clip, head, sd = _setup(spec, size, word_len)
    img, word = _inputs(B, B, size, word_len)
    r = InferenceRunner(clip, head, sd, DEV, fold_bn=fold, use_graph=False)
    a = r(img, word).clone()
    s = r.segment(img, word, list(range(B))).clone()
    torch.cuda.synchronize()
    assert s.shape == a.shape == (B, 1, size // 4, size // 4)
    assert torch.equal(s, a)


@pytest.mark.parametrize("fold", [True, False])
def test_permutations_are_exact(fold):
    clip, head, sd = _setup("tiny", 96, 9)
    B, K = 3, 6
    img, word = _inputs(B, K, 96, 9)
    r = InferenceRunner(clip, head, sd, DEV, fold_bn=fold, use_graph=False)
    idx = torch.tensor([2, 0, 2, 1, 0, 2])
    word[5] = word[0]                                # (image 2, word 0) twice: rows 0 and 5
    base = r.segment(img, word, idx).clone()
    # permuting the expressions (word rows and index together) permutes the output rows
    perm = torch.tensor([4, 1, 5, 0, 3, 2])
    p1 = r.segment(img, word[perm.to(DEV)], idx[perm]).clone()
    # permuting the images and remapping the index leaves the output unchanged
    iperm = torch.tensor([1, 2, 0])                  # new image j = old image iperm[j]
    inv = torch.argsort(iperm)
    p2 = r.segment(img[iperm.to(DEV)], word, inv[idx]).clone()
    torch.cuda.synchronize()
    assert torch.equal(p1, base[perm.to(DEV)])
    assert torch.equal(p2, base)
    assert torch.equal(base[0], base[5])


@pytest.mark.parametrize("spec,B,K,size,word_len", [("tiny", 2, 5, 96, 9), ("r50", 2, 3, 416, 17)])
def test_against_gathered_batch(spec, B, K, size, word_len):
    """any pairing of images and expressions against the batch forward on the gathered images.  The image stage runs at M = B,
    the batch forward at M = K: another tile variant may run there.  The library keeps the k order of every variant, and the two
    came out bit-identical on MI355X (tiny and R50) - printed, not asserted"""
    clip, head, sd = _setup(spec, size, word_len)
    idx = [1, 0, 1, 1, 0][:K]
    r = InferenceRunner(clip, head, sd, DEV, use_graph=False)
    img, word = _inputs(B, K, size, word_len)
    s = r.segment(img, word, idx).clone()
    g = r(img[torch.tensor(idx, device=DEV)], word).clone()
    torch.cuda.synchronize()
    e = _rel(s.cpu(), g.cpu())
    print("segment vs runner(img[index]) %.3e (bitwise: %s)" % (e, torch.equal(s, g)))
    assert s.shape == g.shape == (K, 1, size // 4, size // 4)
    assert e < 3e-2, e


@pytest.mark.parametrize("spec,B,idx,size,word_len", [("tiny", 3, [2, 0, 1, 2, 0], 96, 9), ("r50", 1, [0, 0, 0], 416, 17)])
def test_against_oracle(spec, B, idx, size, word_len):
    """the CPU oracle, at the bound tests/test_infer_gpu.py holds the folded batch forward to (rel. L2 over the whole output), on
    ITS inputs (synth.make_batch(B, ..., 0, 0)), every image paired with its own expression.  Per expression the tiny pairs here
    measured 4.6e-3 .. 2.1e-2.  On the random pairings of test_against_gathered_batch the batch forward itself measured up to
    3.6e-2 (tiny) and 5.6e-2 .. 7.1e-2 (R50) per expression from the oracle on these synthetic weights, with segment bit-identical
    to it: that spread belongs to the bf16 path and its input, not to the gathers."""
    clip, head, sd = _setup(spec, size, word_len)
    img, word, _ = synth.make_batch(B, size, word_len, 0, 0)
    ti = torch.tensor(idx)
    r = InferenceRunner(clip, head, sd, DEV, use_graph=False)
    s = r.segment(img.to(DEV), word[ti].to(DEV), idx).clone()
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = O.cris_forward(sd, clip, head, img[ti], word[ti], training=False)
    assert s.shape == ref.shape == (len(idx), 1, size // 4, size // 4)
    e = _rel(s.cpu(), ref)                          # over the whole output, as tests/test_infer_gpu.py measures it
    print("segment vs oracle %.3e (per expression %s)" % (e, " ".join("%.3e" % _rel(s[k].cpu(), ref[k]) for k in range(len(idx)))))
    assert e < 2e-2, e


def test_graph_replay_equals_eager_and_upsample():
    clip, head, sd = _setup("tiny", 64, 9)
    g = InferenceRunner(clip, head, sd, DEV, use_graph=True)
    e = InferenceRunner(clip, head, sd, DEV, use_graph=False)
    u = InferenceRunner(clip, head, sd, DEV, use_graph=True, upsample=True)
    B, K = 2, 5
    for t in range(5):
        img, word = _inputs(B, K, 64, 9, step=t)
        idx = torch.randint(0, B, (K,), generator=torch.Generator().manual_seed(t))     # a new index content every call
        a, b = g.segment(img, word, idx).clone(), e.segment(img, word, idx).clone()
        p = u.segment(img, word, idx.tolist()).clone()
        torch.cuda.synchronize()
        assert torch.equal(a, b), t
        assert p.shape == (K, 64, 64) and torch.equal(p, evalpost.sigmoid_upsample(b, 64, 64)), t
    assert g.graph_error is None and u.graph_error is None
    assert len(g._shapes) == 1 and next(iter(g._shapes.values()))["graph"] is not None


def test_module_segment_expressions():
    from cris.pytorch_amd.model import build_segmenter
    from test_module_surface import TINY
    model, groups = build_segmenter(NS(**TINY))
    clip, head = arch.specs_by_name("tiny")
    model.load_state_dict(arch.synthetic_state_dict(clip, head, 0))
    model = model.to(DEV).eval()
    img, word, mask = (t.to(DEV) for t in synth.make_batch(4, 64, 9, 0, 0))
    a = model.segment_expressions(img, word, [0, 1, 2, 3])
    b = model(img, word)
    assert torch.equal(a, b)
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.segment_expressions(img, word, [0, 1, 2, 3])
    opt = torch.optim.Adam(groups, lr=1e-3, weight_decay=0.0)
    _, _, loss = model(img, word, mask)
    opt.zero_grad()
    loss.backward()
    opt.step()
    model.eval()
    a2 = model.segment_expressions(img, word, [0, 1, 2, 3])
    b2 = model(img, word)
    assert torch.equal(a2, b2)
    assert not torch.equal(a2, a)                    # the new weights are what ran
    # a returned tensor is the caller's: the next call does not overwrite it
    keep = a2.clone()
    model.segment_expressions(img, word[[1, 0, 3, 2]], [0, 0, 0, 0])
    assert torch.equal(a2, keep)
