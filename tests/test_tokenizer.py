"""BPE tokenizer (cris/pytorch_amd/tokenizer.py) against the reference's own (utils/simple_tokenizer.py + utils/dataset.py
tokenize), bit exact: against its answers stored in tests/golden/tokenizer_reference.json.gz and the known answers of
tests/golden/tokenizer_vectors.json (both written by the reference tokenizer, tests/golden/make_golden.py), with the part of the
CLIP merge list that both tokenizers read (tests/golden/clip_bpe_merges.txt.gz)."""
import gzip
import json
import os

import pytest
import torch

from conftest import GOLDEN
from cris.pytorch_amd import tokenizer as T

MERGES = os.path.join(GOLDEN, "clip_bpe_merges.txt.gz")


@pytest.fixture(scope="module")
def tok():
    return T.BPETokenizer(MERGES, fix_text=lambda s: s)          # (the reference answered with the same ftfy stand-in)


@pytest.fixture(scope="module")
def ref():
    with gzip.open(os.path.join(GOLDEN, "tokenizer_reference.json.gz"), "rt", encoding="utf-8") as f:
        return json.load(f)


def test_known_answers(tok):
    for v in json.load(open(os.path.join(GOLDEN, "tokenizer_vectors.json"))):
        ids = tok.tokenize(v["text"], v["context_length"], True)[0]
        assert ids.tolist() == v["ids"], v["text"]
        assert int(ids.argmax()) == v["argmax"]
    assert (tok.sot, tok.eot, len(tok.words)) == (49406, 49407, 49408)


def test_equals_reference_tokenizer(tok, ref):
    """3000 seeded referring-expression sentences and edge cases at context lengths 17 / 22 / 77, the over-long text error,
    encode / decode of the first 300"""
    texts = ref["texts"]
    for L in (17, 22, 77):
        got = tok.tokenize(texts, L, True)
        assert str(got.dtype) == ref["dtype"]
        want = torch.tensor(ref["ids"][str(L)], dtype=got.dtype)
        bad = (want != got).any(dim=1).nonzero().flatten().tolist()
        assert not bad, [(texts[i], want[i].tolist(), got[i].tolist()) for i in bad[:3]]
    # no truncation: same error behaviour
    with pytest.raises(RuntimeError, match="too long"):
        tok.tokenize("x " * 40, 17, False)
    assert "too long" in ref["too_long_error"]
    # the raw id lists and the round trip
    assert len(ref["encode"]) == len(ref["decode"]) == 300
    for t, ids, back in zip(texts, ref["encode"], ref["decode"]):
        assert tok.encode(t) == ids
        assert tok.decode(ids) == back


def test_without_ftfy_non_ascii_is_refused_not_mangled():
    t = T.BPETokenizer(MERGES)
    try:
        import ftfy  # noqa: F401
        has = True
    except ImportError:
        has = False
    if has and getattr(__import__("ftfy"), "__file__", None):
        pytest.skip("ftfy installed")
    if t._fix is T._ascii_only_repair:
        assert t.tokenize("a plain ascii sentence", 17, True).shape == (1, 17)
        with pytest.raises(RuntimeError, match="ftfy"):
            t.tokenize("café", 17, True)


def test_property_any_text_tokenizes_like_the_reference(tok, ref):
    """arbitrary unicode text (control characters included, surrogates excluded), any context length: the 400 cases hypothesis
    drew (derandomized) for the fixture, with the reference's answers"""
    cases = ref["hypothesis"]
    assert len(cases) >= 400
    for c in cases:
        got = tok.tokenize(c["text"], c["L"], True)
        assert got.shape == (1, c["L"]) and got[0].tolist() == c["ids"], (c["text"], c["ids"], got.tolist())
