"""Host side of the dataset evaluation (cris/pytorch_amd/evaluate.py, evalpost.EvalStaging; reference engine/engine.py:90-215):
the metrics against the reference's torch expressions, the shard arithmetic against DistributedSampler, the descriptor and
mask packing on the staging buffer, and the count gather over a world-size-2 gloo group.  No GPU."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def _reference_metrics(iou_list):
    """engine.py:125-143 as written there (iou_list: the float64 array np.stack makes)"""
    iou_list = torch.from_numpy(np.stack(iou_list))
    prec_list = []
    for thres in torch.arange(0.5, 1.0, 0.1):
        tmp = (iou_list > thres).float().mean()
        prec_list.append(tmp)
    iou = iou_list.mean()
    prec = {}
    for i, thres in enumerate(range(5, 10)):
        prec['Pr@{}'.format(thres * 10)] = prec_list[i].item()
    return iou.item(), prec


def _counts_with_iou(target):
    """(inter, union) whose inter / (union + 1e-6) is as close to `target` as integers allow"""
    union = 1000000
    return [int(round(target * (union + 1e-6))), union]


def test_metrics_match_the_reference_expressions():
    from cris.pytorch_amd import evaluate
    ths = evaluate.pr_thresholds()
    assert ths == [float(np.float32(v)) for v in torch.arange(0.5, 1.0, 0.1).tolist()] and len(ths) == 5
    assert ths[1] > 0.6 and ths[1] == float(np.float32(0.6))          # 0.6f widened is ABOVE the double 0.6
    # integer tables around every threshold, empty masks (0 / 0), full agreement
    table = [[0, 0], [5, 5], [0, 9], [1, 3]]
    for t in (0.5, 0.6, 0.7, 0.8, 0.9):
        for d in (-2, -1, 0, 1, 2):
            table.append(_counts_with_iou(t + d * 1e-6))
    rng = np.random.default_rng(0)
    u = rng.integers(1, 300000, 200)
    table += [[int(rng.integers(0, v + 1)), int(v)] for v in u]
    iou, prec, per = evaluate.metrics(table)
    ref_list = [np.sum(i) / (np.sum(un) + 1e-6) for i, un in table]       # engine.py:123 on integer sums
    ref_iou, ref_prec = _reference_metrics(ref_list)
    assert np.array_equal(per, np.asarray(ref_list))
    assert list(prec) == ["Pr@50", "Pr@60", "Pr@70", "Pr@80", "Pr@90"]
    assert prec == ref_prec                                               # counts of comparisons and a float32 quotient: exact
    assert abs(iou - ref_iou) <= len(table) * 2.0 ** -52 * max(ref_iou, 1.0)   # float64 sums of n terms in another order
    # the comparison itself, on IoU VALUES placed exactly: the double 0.6, float32(0.6) widened, and their neighbours
    f = float(np.float32(0.6))
    vals = np.array([0.6, np.nextafter(0.6, 1), f, np.nextafter(f, 0), np.nextafter(f, 1), 0.5, np.nextafter(0.5, 1),
                     float(np.float32(0.9)), np.nextafter(float(np.float32(0.9)), 1), 0.9, 0.7, float(np.float32(0.7)), 0.8,
                     float(np.float32(0.8))])
    for k, t in zip(evaluate.PR_KEYS, torch.arange(0.5, 1.0, 0.1)):
        want = (torch.from_numpy(vals) > t).tolist()
        got = (vals > evaluate.pr_thresholds()[evaluate.PR_KEYS.index(k)]).tolist()
        assert got == want, k
    assert not (0.6 > evaluate.pr_thresholds()[1]) and not (f > evaluate.pr_thresholds()[1]) and np.nextafter(f, 1) > evaluate.pr_thresholds()[1]
    # through metrics(): one sample per value is not reachable with integer counts, so check the rule metrics applies
    one = evaluate.metrics([[6, 10]])                                     # 6 / (10 + 1e-6) < 0.6
    assert one[1]["Pr@50"] == 1.0 and one[1]["Pr@60"] == 0.0
    with pytest.raises(ValueError):
        evaluate.metrics(np.zeros((0, 2)))


@pytest.mark.parametrize("n", [10, 16, 17])
@pytest.mark.parametrize("world", [1, 2, 8])
def test_shard_indices_equal_distributed_sampler(n, world):
    from torch.utils.data.distributed import DistributedSampler
    from cris.pytorch_amd import evaluate
    for rank in range(world):
        assert evaluate.shard_indices(n, rank, world) == list(DistributedSampler(range(n), world, rank, shuffle=False))
    with pytest.raises(ValueError):
        evaluate.shard_indices(n, world, world)


def _mask(rng, h, w):
    return torch.from_numpy((rng.random((h, w)) > 0.5).astype(np.uint8) * 255)


def _inv(i):
    return np.array([[1.2 + 0.1 * i, 0.0, -3.5], [0.0, 1.2 + 0.1 * i, 2.25 - i]], np.float64)


def _check_masks(st, masks, offsets):
    buf = st.host.numpy()
    used = np.zeros(st.mask_bytes, bool)
    for m, off in zip(masks, offsets):
        h, w = m.shape
        pitch = (w + 3) // 4 * 4
        rows = buf[st.mask_base + off:st.mask_base + off + pitch * h].reshape(h, pitch)
        assert np.array_equal(rows[:, :w], m.numpy())
        assert not rows[:, w:].any()                                      # padding bytes are zero
        assert not used[off:off + pitch * h].any()                        # masks do not overlap
        used[off:off + pitch * h] = True
        assert off % 4 == 0 and off + pitch * h <= st.mask_bytes


def test_staging_packs_descriptors_and_masks(built):
    from cris.pytorch_amd import evalpost, evaluate, hip
    from oracle import eval_post as EP
    rng = np.random.default_rng(1)
    sizes = [(33, 25), (5, 3), (1, 1), (48, 64)]                          # widths 25, 3, 1: not multiples of 4
    masks = [_mask(rng, h, w) for h, w in sizes]
    invs = [_inv(i) for i in range(4)]
    # --- validate: batch of 6 holding 4 real samples (the padding repeats the last sample on the device; no descriptor for it)
    st = evalpost.EvalStaging(None, max_descs=2, mask_bytes=64)            # too small on purpose: pack() grows it
    st.host.fill_(0xEE)
    st.pack(*evaluate.plan_validate(masks, invs, row0=0))
    assert st.n == 4 and st.max_descs >= 4
    offs = [st.descs[i].mask_off for i in range(4)]
    _check_masks(st, masks, offs)
    for i, (h, w) in enumerate(sizes):
        d = st.descs[i]
        assert (d.w_out, d.h_out, d.map, d.row) == (w, h, i, i)
        assert d.pitch % 4 == 0 and w <= d.pitch < w + 4
        assert np.array_equal(np.array(d.m[:]).reshape(2, 3), EP.invert_affine(invs[i]))      # destination -> source, in double
    assert len(set(offs)) == 4
    assert C.sizeof(hip.EvalDesc) * st.max_descs <= st.mask_base and st.mask_base % 16 == 0
    # --- inference: 3 images with 2, 1, 3 sentences -> K = 6, padded to 8 by repeating the last expression
    index, m3, descs = evaluate.plan_inference(masks[:3], invs[:3], [2, 1, 3])
    assert index == [0, 0, 1, 2, 2, 2, 2, 2] and len(descs) == 6          # padded K: no extra descriptor
    st.pack(m3, descs)
    assert st.n == 6
    d = [st.descs[k] for k in range(6)]
    assert [x.map for x in d] == [0, 1, 2, 3, 4, 5] and [x.row for x in d] == [0, 1, 2, 3, 4, 5]
    assert d[0].mask_off == d[1].mask_off and d[3].mask_off == d[4].mask_off == d[5].mask_off      # expressions of one image share its mask
    assert len({d[0].mask_off, d[2].mask_off, d[3].mask_off}) == 3
    _check_masks(st, m3, [d[0].mask_off, d[2].mask_off, d[3].mask_off])
    assert len({x.out_off for x in d}) == 6                               # but every expression has an output of its own
    assert st.out_bytes >= sum(x.pitch * x.h_out for x in d)
    # K already a multiple of 8: nothing is added
    index, _, descs = evaluate.plan_inference(masks[:2], invs[:2], [3, 5])
    assert index == [0] * 3 + [1] * 5 and len(descs) == 8


def test_launcher_rejects_bad_geometry_on_the_host(built):
    """cris_eval_iou_batch checks every descriptor against the buffers before it touches the device"""
    from cris.pytorch_amd import hip
    l = hip.load()
    d = (hip.EvalDesc * 1)()
    mat = (C.c_double * 6)(1, 0, 0, 0, 1, 0)

    def launch(mask_bytes=1 << 20, rows=4, out=None, out_bytes=0):
        return l.cris_eval_iou_batch(0x1000, 2, 8, 8, C.addressof(d), 0x2000, 1, 0x3000, mask_bytes, 0.35, 0.0, 0x4000, rows, out, out_bytes, None)

    cases = [dict(w=46341, h=46341, pitch=46344), dict(w=0, h=4), dict(w=5, h=4, pitch=6), dict(w=5, h=4, pitch=4), dict(w=5, h=4, map=2),
             dict(w=5, h=4, row=4), dict(w=5, h=4, mask_off=2), dict(w=5, h=4, mask_off=(1 << 20) - 16)]
    for c in cases:
        w, h = c["w"], c["h"]
        assert l.cris_eval_desc_fill(C.addressof(d), mat, w, h, c.get("map", 0), c.get("mask_off", 0), c.get("pitch", (w + 3) // 4 * 4), 0,
                                     c.get("row", 0)) == 0
        assert launch(mask_bytes=1 << 40 if w > 40000 else 1 << 20) != 0 and b"descriptor" in l.cris_last_error(), c
    assert l.cris_eval_desc_fill(C.addressof(d), mat, 5, 4, 0, 0, 8, 64, 0) == 0
    assert launch(out=0x5000, out_bytes=64) != 0 and b"output outside" in l.cris_last_error()
    assert l.cris_eval_iou_batch(0x1000, 2, 8, 8, C.addressof(d), 0x2000, 1, 0x3001, 64, 0.35, 0.0, 0x4000, 4, None, 0, None) != 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _table(n):
    rng = np.random.default_rng(3)
    union = rng.integers(1, 100000, n)
    return np.stack([(union * rng.random(n)).astype(np.int64), union], 1).astype(np.int32)


def _worker(rank, world, port, n, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cris.pytorch_amd import evaluate
        full = _table(n)
        mine = torch.from_numpy(full[evaluate.shard_indices(n, rank, world)])
        got = evaluate.gather_counts(mine)                                # no group given: the default group is found
        got2 = evaluate.gather_counts(mine, dist.group.WORLD)
        q.put((rank, got.numpy().tolist(), torch.equal(got, got2)))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_gathered_counts_give_the_single_process_metrics():
    from cris.pytorch_amd import evaluate
    n, world = 7, 2                                                       # odd: rank 1's shard wraps around to sample 0
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    full = _table(n)
    concat = np.concatenate([full[evaluate.shard_indices(n, r, world)] for r in range(world)])     # concat_all_gather: rank order
    assert concat.shape[0] == 8
    want = evaluate.metrics(concat)
    for rank, got, same in res:
        assert same
        assert np.array_equal(np.asarray(got), concat), rank
        m = evaluate.metrics(np.asarray(got))
        assert m[0] == want[0] and m[1] == want[1] and np.array_equal(m[2], want[2])
    # without a process group the table comes back as it is
    t = torch.from_numpy(full)
    assert evaluate.gather_counts(t) is t
