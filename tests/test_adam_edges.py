"""The fused multi-tensor update at its block, tile and table edges, element by element: adam_kernel<PT, MODE>, adam_pack_tile,
unpack_grads_kernel and grad_sumsq_kernel of csrc/elementwise.hip through ops.AdamTable / ops.UnpackTable.

One step from a state the test wrote, every element of p', m' and v' against the float64 statement of the step under the derived
bounds of tests/adam_edge_cases.py (which also holds the case tables and the layout statements; tests/test_adam_edges_cpu.py shows
that a plain fp32 evaluation meets the bounds and that wrong ones do not).  p, g, m, v, both packs and the row marks are windows
of guarded slabs: outputs lie in GUARD_BITS that must survive every launch, inputs in NaN, padding columns of GEMM-layout
gradients and gradients of rows without one hold NaN.  The tables are built by ops.AdamTable, so its descriptor filling is part
of what is tested; m and v are then pointed at guarded buffers (the way set_lrs rewrites a table), the packs are allocated here.

Worst error / bound on an MI355X (printed per table by test_one_step): m' 0.156, v' 0.261, p' 0.149 over all tables - the
coupled ones; without coupled decay m' 0.114, v' 0.158, p' 0.149.  The fp32 evaluation on the CPU: m' 0.156, v' 0.261, p' 0.145.
The 23 tests take 4 s together, the slowest (a table of 257 tensors, 1500 small buffers) 0.4 s."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import hip, ops  # noqa: E402
import adam_edge_cases as A  # noqa: E402
from hip_ops_edge_cases import BF, F32, Slab, assert_exact, bits_equal  # noqa: E402

DEV = "cuda"
PAD = 8                             # guard elements on either side of a flat window
_WORST = {}


def window(n, dtype, values=None, nan_guard=False):
    """n elements inside one guarded row (and a guard row in front and behind); .flat is what the kernel gets"""
    s = Slab(1, n, dtype, DEV, ld=n + 2 * PAD, coff=PAD, nan_guard=nan_guard, pre=1, post=1)
    if values is not None:
        s.set(values)
    s.flat = s.data.view(-1)
    assert s.flat.data_ptr() == s.data.data_ptr()
    return s


class Table:
    """an ops.AdamTable over guarded windows, holding the state of `case`"""

    def __init__(self, case):
        self.case = case
        self.states = [A.state(case, k) for k in range(len(case.tensors))]
        self.p, self.g, self.m, self.v, self.F, self.D, self.live = [], [], [], [], {}, {}, {}
        params, grads, packs, row_live = [], [], [], {}
        for k, (t, st) in enumerate(zip(case.tensors, self.states)):
            self.p.append(window(t.numel, F32, st["p"]))
            self.m.append(window(t.numel, F32, st["m"]))
            self.v.append(window(t.numel, F32, st["v"]))
            self.g.append(window(t.grad_numel, F32, st["gbuf"], nan_guard=True))
            params.append(self.p[k].flat.view(t.dims) if t.kind == "rows" else self.p[k].flat)
            grads.append(self.g[k].flat)
            pk = None
            if t.kind == "pack":
                if t.want_F:
                    self.F[k] = Slab(t.N, t.ldF, BF, DEV, pre=A.PRE, post=A.POST)
                if t.want_D:
                    self.D[k] = Slab(t.Cin, t.ldD, BF, DEV, pre=A.PRE, post=A.POST)
                f, d = self.F.get(k), self.D.get(k)
                pk = (f.rows if f else None, d.rows if d else None, t.N, t.Cin, t.taps, t.Cpad, t.Npad, t.transposed)
            packs.append(pk)
            if t.dead:
                marks = torch.ones(t.N, dtype=torch.uint8)
                marks[list(t.dead)] = 0
                self.live[k] = window(t.N, torch.uint8, marks)
                row_live[k] = self.live[k].flat
        self.tab = ops.AdamTable(params, grads, case.lrs, layouts=[t.layout for t in case.tensors], packs=packs, row_live=row_live or None)
        for taps, idx in self.tab.index.items():                    # state in guarded buffers instead of the table's zeros
            tt = self.tab.tables[taps]
            for j, i in enumerate(idx):
                tt.arr[j].m, tt.arr[j].v = self.m[i].flat.data_ptr(), self.v[i].flat.data_ptr()
                self.tab.m[i], self.tab.v[i] = self.m[i].flat, self.v[i].flat
            tt.upload(DEV)
        if case.mode:
            self.tab.set_decay(case.decays, case.mode == 2)
        torch.cuda.synchronize()

    def slabs(self):
        """(name, slab) of every buffer the launches may or may not write"""
        for k, t in enumerate(self.case.tensors):
            for key, group in (("p", self.p), ("g", self.g), ("m", self.m), ("v", self.v)):
                yield "%s/%s slab %s" % (self.case.name, t.name, key), group[k]
            for key, group in (("pack F", self.F), ("pack D", self.D), ("row_live", self.live)):
                if k in group:
                    yield "%s/%s slab %s" % (self.case.name, t.name, key), group[k]

    def images(self):
        torch.cuda.synchronize()
        return {name: s.full.cpu().clone() for name, s in self.slabs()}

    def step(self):
        c = self.case
        args = dict(beta1=A.B1, beta2=A.B2, eps=A.EPS, weight_decay=c.wd, grad_scale=c.gscale)
        if c.step_dev:
            self.tab.step_count = 100                               # the host counter is wrong on purpose: the device's must win
            args["step_dev"] = torch.tensor([c.t], dtype=torch.int32, device=DEV)
        else:
            self.tab.step_count = c.t - 1
        if c.loss_scale is not None:
            args["loss_scale_dev"] = torch.tensor([c.loss_scale], dtype=torch.float32, device=DEV)
        if c.skip:
            args["skip_dev"] = torch.tensor([1.0], dtype=torch.float32, device=DEV)
        self.tab.step(**args)
        torch.cuda.synchronize()

    def result(self):
        out = []
        for k, t in enumerate(self.case.tensors):
            r = dict(p=self.p[k].get().flatten(), m=self.m[k].get().flatten(), v=self.v[k].get().flatten())
            if k in self.F:
                r["F"] = self.F[k].full.cpu().view(torch.int16).clone()
            if k in self.D:
                r["D"] = self.D[k].full.cpu().view(torch.int16).clone()
            out.append(r)
        return out

    def assert_guards(self, before):
        """guards of the fp32 outputs (the packs' are checked against the layout statements by A.check), inputs untouched"""
        for name, s in self.slabs():
            if name.endswith((" p", " m", " v")):
                s.assert_guards(name)
            elif name.endswith((" g", " row_live")):
                assert bits_equal(s.full.cpu(), before[name]), "%s: an input was written" % name


def test_block_size_is_the_one_the_cases_assume():
    assert hip.load().cris_adam_block_elems() == A.BLOCK_ELEMS


@pytest.mark.parametrize("case", A.CASES, ids=repr)
def test_one_step(case):
    """p', m', v' per element within the bounds, packs bit for bit from p', guards intact; before the step, cris_grad_sumsq per
    tensor over the same (NaN-padded) gradients"""
    tb = Table(case)
    before = tb.images()
    check_grad_sumsq(tb)
    after_norm = tb.images()
    for name in before:
        assert bits_equal(after_norm[name], before[name]), "%s: written by cris_grad_sumsq" % name
    tb.step()
    tb.assert_guards(before)
    if case.skip:
        after = tb.images()
        for name in before:
            assert bits_equal(after[name], before[name]), "%s: changed by a skipped step" % name
    report = {}
    A.check(case, tb.states, tb.result(), report)
    for key, r in report.items():
        _WORST[key] = max(_WORST.get(key, 0.0), r)
    print("%s: worst error / bound on the GPU: %s; over the tables so far: %s" % (
        case.name, " ".join("%s' %.3f" % kv for kv in sorted(report.items())), " ".join("%s' %.3f" % kv for kv in sorted(_WORST.items()))))


def check_grad_sumsq(tb):
    """the per-tensor check of test_grad_clip_gpu.py::test_each_tensor_sums_over_its_own_blocks: the partials of every tensor's own
    block range, added in double, equal the float64 sum of squares of its logical gradient to 1e-5 (derived there).  Padding and
    the gradients of rows without one hold NaN: one stray read makes the sum NaN."""
    tab = tb.tab
    tab.grad_norm()
    partials = tab._partials.cpu().double()
    want = A.grad_sumsq_reference(tb.states)
    off = 0
    for taps in (9, 1):
        t, idx = tab.tables[taps], tab.index[taps]
        for j, i in enumerate(idx):
            lo = t.arr[j].block_start
            hi = t.arr[j + 1].block_start if j + 1 < len(idx) else t.total_blocks
            got = float(partials[off + lo:off + hi].sum())
            assert hi > lo and abs(got - want[i]) <= 1e-5 * want[i], "%s/%s: sum of squares over blocks %d..%d: got %r, float64 %r" % (
                tb.case.name, tb.case.tensors[i].name, lo, hi, got, want[i])
        off += t.total_blocks if t.n else 0
    assert off == tab._partials.numel()


@pytest.mark.parametrize("name", sorted(A.UNPACK_CASES))
def test_unpack_grads(name):
    """cris_unpack_grads: the destination is the layout statement's reading of the source, bit for bit; padding NaN, guards intact"""
    tensors = A.UNPACK_CASES[name]
    srcs, dsts, want = [], [], []
    for k, t in enumerate(tensors):
        g = torch.randn(t.numel, generator=torch.Generator().manual_seed(500 + k))
        buf = torch.full((t.grad_numel,), A.NAN)
        buf[A.gemm_index(t)] = g
        want.append(g)
        srcs.append(window(t.grad_numel, F32, buf, nan_guard=True))
        dsts.append(window(t.numel, F32))
    tab = ops.UnpackTable([s.flat for s in srcs], [d.flat for d in dsts], [t.layout for t in tensors])
    assert tab.n == len(tensors)
    tab.run()
    torch.cuda.synchronize()
    for t, d, w in zip(tensors, dsts, want):
        what = "unpack %s/%s" % (name, t.name)
        d.assert_guards(what + " slab dst")
        assert_exact(d.get().view(t.dims), w.view(t.dims), what, names=t.names)
