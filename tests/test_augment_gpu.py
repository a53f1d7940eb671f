"""Training-time augmentation of the GPU input pipeline on the device: the geometry against the restated OpenCV warps, the colour
steps against their numpy restatement (tests/augment_cases.py) - both bit for bit, every step is one IEEE float32 operation - the
two rules that keep un-augmented pixels what they were, the luminance sums, and RecordPipeline end to end.  Small ragged shapes:
a non-square 36 x 52 network input (1872 pixels, not a multiple of the 256-thread block), sources down to 1 x 1."""
import ctypes as C
import io
import pickle

import numpy as np
import pytest
import torch

import augment_cases as ac
from cris.pytorch_amd import hip, inputpipe, records
from cris.pytorch_amd.inputpipe import Augment, AugmentParams, Preprocessor, augment_matrix
from oracle import input_pipe as ip

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
S = ac.INPUT_SIZE


def _geometry():
    """one of each per sample: zoom out + rotation (border on all sides), zoom in (crop), shift, mirror, identity"""
    return [dict(scale=0.6, angle=17.0), dict(scale=1.7), dict(tx=0.2 * S[1], ty=0.2 * S[0]), dict(flip=True), dict()]


@pytest.fixture(scope="module")
def setup():
    imgs, masks = ac.batch()
    return Preprocessor(S, DEV), imgs, masks


def _check(pre, imgs, masks, params):
    img, mask, mats, invs = pre(imgs, masks, params)
    torch.cuda.synchronize()
    img, mask = img.cpu().numpy(), mask.cpu().numpy()
    for i, p in enumerate(params):
        M = augment_matrix(imgs[i].shape[:2], S, p)
        assert np.array_equal(mats[i], M) and np.array_equal(pre.last_params[i].mat, M)
        want = ac.reference_image(imgs[i], M, S, p.fb, p.fc, p.fs)
        assert np.array_equal(img[i], want), (i, p, int((img[i] != want).sum()), float(np.abs(img[i] - want).max()))
        if masks[i] is not None:
            assert np.array_equal(mask[i], ac.reference_mask(masks[i], M, S)), (i, p)
        else:
            assert float(np.abs(mask[i]).max()) == 0.0
    return img, mask


def test_geometry_is_bit_exact_against_the_restated_warps(setup):
    pre, imgs, masks = setup
    params = [AugmentParams(**g) for g in _geometry()]
    img, mask = _check(pre, imgs, masks, params)
    # the returned inverse is the destination->source map the kernel used
    _, _, mats, invs = pre(imgs, masks, params)
    for mt, inv in zip(mats, invs):
        full = np.vstack([mt, [0, 0, 1]]) @ np.vstack([inv, [0, 0, 1]])
        assert inv.shape == (2, 3) and np.allclose(full, np.eye(3), atol=1e-9)
    # the rotated, shrunk sample really has border on all four sides and image in the middle
    border = ip.convert_image(np.broadcast_to(ip.border_u8(ip.BORDER_RGB, 3), (1, 1, 3)))[:, 0, 0]
    for y, x in ((0, 0), (0, S[1] - 1), (S[0] - 1, 0), (S[0] - 1, S[1] - 1)):
        assert np.array_equal(img[0][:, y, x], border)
    assert not np.array_equal(img[0][:, S[0] // 2, S[1] // 2], border)


def test_colour_is_bit_exact_against_the_numpy_restatement(setup):
    pre, imgs, masks = setup
    geo = _geometry()
    no_contrast = [ac.TRIPLES[i] for i in (1, 4, 5, 0, 7)]          # no fc != 1 in the batch: no luminance pass, sums = NULL
    for triples, shift in ((ac.TRIPLES[0:5], 0), (ac.TRIPLES[3:8], 2), (ac.TRIPLES[5:8] + ac.TRIPLES[1:3], 4), (no_contrast, 1)):
        params = [AugmentParams(fb=t[0], fc=t[1], fs=t[2], **geo[(i + shift) % 5]) for i, t in enumerate(triples)]
        _check(pre, imgs, masks, params)


def test_identity_sample_of_a_mixed_batch_is_the_plain_call(setup):
    pre, imgs, masks = setup
    plain_img, plain_mask, plain_mats, _ = pre(imgs, masks)
    params = [AugmentParams(scale=0.6, angle=17.0, fb=0.75, fc=1.3, fs=0.6), AugmentParams(), AugmentParams(fc=0.5), AugmentParams(),
              AugmentParams(flip=True, fs=1.5)]
    img, mask, mats, _ = pre(imgs, masks, params)
    torch.cuda.synchronize()
    for i in (1, 3):
        assert torch.equal(img[i], plain_img[i]) and torch.equal(mask[i], plain_mask[i]) and np.array_equal(mats[i], plain_mats[i])
    for i in (0, 2, 4):
        assert not torch.equal(img[i], plain_img[i])
    # an all-identity parameter list is the plain call, bit for bit
    img2, mask2, _, _ = pre(imgs, masks, [AugmentParams()] * len(imgs))
    torch.cuda.synchronize()
    assert torch.equal(img2, plain_img) and torch.equal(mask2, plain_mask)


def test_pure_border_stays_the_normalised_border(setup):
    pre, imgs, masks = setup
    plain, _, mats, _ = pre(imgs, masks, [AugmentParams(scale=0.3)] * len(imgs))          # geometry only: cris_preprocess_batch
    dark, _, _, _ = pre(imgs, masks, [AugmentParams(scale=0.3, fb=0.5)] * len(imgs))
    torch.cuda.synchronize()
    plain, dark = plain.cpu().numpy(), dark.cpu().numpy()
    border = ip.convert_image(np.broadcast_to(ip.border_u8(ip.BORDER_RGB, 3), (1, 1, 3)))[:, 0, 0]
    for i, im in enumerate(imgs):
        outside = ~ac.taps_inside(mats[i], im.shape[:2], S)
        assert outside.any() and not outside.all(), i
        assert np.array_equal(dark[i][:, outside], plain[i][:, outside])
        assert np.array_equal(dark[i][:, outside], np.broadcast_to(border[:, None], (3, int(outside.sum()))))
        assert not np.array_equal(dark[i][:, ~outside], plain[i][:, ~outside])


def _gray_sums(imgs, calls=1):
    keep = [torch.from_numpy(np.ascontiguousarray(im)).to(DEV) for im in imgs]
    descs = (hip.SampleDesc * len(imgs))()
    for d, t in zip(descs, keep):
        d.img, d.H, d.W = t.data_ptr(), int(t.shape[0]), int(t.shape[1])
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    sums = torch.zeros(len(imgs), dtype=torch.int64, device=DEV)
    for _ in range(calls):
        hip.call("cris_gray_sum_batch", C.addressof(descs), hip.ptr(table), len(imgs), hip.ptr(sums), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return sums.cpu().tolist()


def test_gray_sum_batch(setup):
    _, imgs, _ = setup
    want = [ac.gray_sum(im) for im in imgs]
    assert _gray_sums(imgs) == want                                               # ragged: 1850, 1850, 15 (tail of 3), 1 and 4096 pixels
    assert _gray_sums(imgs, calls=2) == [2 * w for w in want]                     # the kernel adds; zeroing is the caller's
    assert _gray_sums([imgs[2]]) == [want[2]] and _gray_sums([imgs[3]]) == [want[3]]
    white = np.full((512, 512, 3), 255, np.uint8)
    assert _gray_sums([white, imgs[0]]) == [512 * 512 * 65280, want[0]] and 512 * 512 * 65280 > 2 ** 32
    for n in (2, 3, 4, 5, 6, 7):                                                  # every tail length, one row
        im = ac.image(1, n, 20 + n)
        assert _gray_sums([im]) == [ac.gray_sum(im)]


# ---- RecordPipeline end to end ---------------------------------------------------------------------------------------------

class _StandInTokenizer:
    """the CLIP merge list is not on the GPU machine: a deterministic stand-in with the tokenizer's interface"""

    def tokenize(self, texts, context_length=77, truncate=False):
        texts = [texts] if isinstance(texts, str) else texts
        out = torch.zeros(len(texts), context_length, dtype=torch.long)
        for i, t in enumerate(texts):
            ids = [49406] + [1 + (sum(map(ord, w)) % 40000) for w in t.lower().split()][:context_length - 2] + [49407]
            out[i, :len(ids)] = torch.tensor(ids)
        return out


@pytest.fixture(scope="module")
def recs():
    pytest.importorskip("PIL")
    from PIL import Image
    import jpeg_cases
    rng = np.random.default_rng(0)
    out = []
    for i, (h, w, kw) in enumerate([(60, 80, dict(quality=85, subsampling=2)), (80, 60, dict(quality=90, subsampling=1)),
                                    (50, 37, dict(quality=75, subsampling=2)), (48, 48, dict(quality=95, subsampling=0))]):
        b = io.BytesIO()
        Image.fromarray(ac.mask(h, w), "L").save(b, "PNG")
        sents = ["the left one", "Rightmost umbrella #%d" % i, "zebra closest 2 us"]
        rec = {"img": jpeg_cases.encode(jpeg_cases._smooth(rng, h, w), **kw), "mask": b.getvalue(), "cat": 1, "seg_id": 1000 + i,
               "img_name": "x.jpg", "num_sents": len(sents), "sents": sents}
        out.append(records.load_record(pickle.dumps(rec, protocol=5)))
    return out


AUG = Augment(scale=(0.8, 1.25), translate=0.1, rotate=10.0, hflip=1.0, brightness=0.2, contrast=0.2, saturation=0.2)


def test_record_pipeline_is_reproducible_and_last_augment_reproduces_it(recs):
    from cris.pytorch_amd import jpegdec, pngdec
    tok, L = _StandInTokenizer(), 17
    pipe = records.RecordPipeline(40, L, DEV, mode="train", tokenizer=tok, augment=AUG)
    img, word, mask = pipe(recs, np.random.default_rng(5))
    params = pipe.last_augment
    img2, word2, mask2 = pipe(recs, np.random.default_rng(5))
    torch.cuda.synchronize()
    assert torch.equal(img, img2) and torch.equal(word, word2) and torch.equal(mask, mask2)
    assert img.shape == (4, 3, 40, 40) and mask.shape == (4, 40, 40) and word.shape == (4, L)
    # exactly one draw of [B, 8] uniforms, before the sentence draws
    crng = ac.CountingRng(5)
    pipe(recs, crng)
    assert crng.calls[0] == ("random", (4, 8)) and [c[0] for c in crng.calls[1:]] == ["integers"] * 4
    # the parameters are augment_params of that draw, and fed back into the Preprocessor they reproduce the batch
    replay = np.random.default_rng(5)
    want = inputpipe.augment_params(AUG, replay.random((4, 8)), (40, 40))
    assert [p for p in params] == want and all(p.mat is not None and p.mat.shape == (2, 3) for p in params)
    assert all(p.flip for p in params) and len({float(p.fb) for p in params}) == 4
    images = jpegdec.decode_batch([r["img"] for r in recs], DEV)
    masks = [pngdec.decode_gray(r["mask"]) for r in recs]
    rimg, rmask, mats, _ = Preprocessor((40, 40), DEV)(images, masks, params)
    torch.cuda.synchronize()
    assert torch.equal(rimg, img) and torch.equal(rmask, mask)
    assert all(np.array_equal(m, p.mat) for m, p in zip(mats, params))
    # hflip = 1: every sentence has left and right exchanged before tokenising
    for b, r in enumerate(recs):
        sent = r["sents"][int(replay.integers(r["num_sents"]))]
        assert word[b].tolist() == tok.tokenize(records.swap_left_right(sent), L, True)[0].tolist()
    swapped = [tok.tokenize(records.swap_left_right(s), L, True)[0].tolist() != tok.tokenize(s, L, True)[0].tolist() for s in recs[0]["sents"]]
    assert swapped == [True, True, False]


def test_no_augmentation_is_the_pipeline_as_it_was(recs):
    tok, L = _StandInTokenizer(), 17
    outs, states = [], []
    for kw in ({}, dict(augment=None), dict(augment=Augment())):
        pipe = records.RecordPipeline(40, L, DEV, mode="train", tokenizer=tok, **kw)
        rng = np.random.default_rng(11)
        outs.append(pipe(recs, rng))
        states.append(rng.bit_generator.state)
        assert pipe.last_augment is None and pipe.augment is None
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
    assert states[1] == states[0] and states[2] == states[0]
    crng = ac.CountingRng(11)
    records.RecordPipeline(40, L, DEV, mode="train", tokenizer=tok)(recs, crng)
    assert [c[0] for c in crng.calls] == ["integers"] * 4                          # no uniforms are drawn
    # and it is the reference arithmetic still
    import jpeg_cases
    for b, r in enumerate(recs):
        want, _, _, _ = ip.preprocess_train(jpeg_cases.pil_decode(r["img"]), None, (40, 40))
        assert np.array_equal(outs[0][0][b].cpu().numpy(), want)
    with pytest.raises(ValueError):
        records.RecordPipeline(40, L, DEV, mode="val", tokenizer=tok, augment=AUG)
