"""Native training step: Engine forward + backward, overlapped gradient all-reduce, fused HIP Adam.

Semantics follow the reference loop (engine/engine.py:37-73, train.py:105-111): Adam(betas 0.9/0.999, eps 1e-8,
weight_decay from the yaml) over two parameter groups built by the `build_segmenter` name rule
(model/__init__.py:36-48); bf16 needs no loss scaling so there is no GradScaler; the train metric
(utils/misc.py:114-129) is computed on the device without a host sync.

Launch model: the step is a static schedule of ~1000 kernel launches.  After one eager step (which fills the host-side
caches and the allocator) the whole step - forward, backward, gradient exchange, Adam, metric - is captured ONCE into a
HIP graph (torch.cuda.CUDAGraph over the launch stream; the independent text-encoder branch is captured on a second
stream and so becomes a parallel branch of the graph) and replayed per step: one host call per step instead of one per
kernel.  What changes from step to step lives in device memory: the input batch (static buffers the caller's tensors
are copied into), the step counter (Adam bias corrections) and the dropout seed (`cris_step_advance`).

With more than one rank the step contains RCCL collectives (SyncBN statistics, gradient exchange).  There the default
launch mode is a host-side COMMAND LIST (hip.CommandList): the second step is executed once more by the Python schedule
while every library call (function pointer + ctypes arguments) and every torch-level op (stream wait, collective) is
recorded, with all of its buffers allocated from a private torch MemPool so their addresses stay valid; later steps
replay the list - a few microseconds of Python per launch, collectives issued by torch.distributed as usual.
`launch=` / CRIS_LAUNCH selects "graph", "cmdlist" or "eager" explicitly.

Gradient accumulation (`accum_steps=K`): train_step takes the whole optimizer batch of K*b samples and runs K forward/backward
passes over its K equal slices from the same parameters - the usual `for chunk: (loss_chunk / K).backward()`, then clip, then
`optimizer.step()`.  The sum is kept in a second arena-sized buffer `acc` and built per arena stage from the backward's stage
hook: acc = g0, acc += g1, ..., and in the last micro-batch g += acc, so the total ((g0 + g1) + g2) + ... + g_{K-1} (one fp32
rounding per add, in this order) ends up in the gradient arena, where the exchange, the norm, Adam and grads_param_layout() read
it.  The 1/K goes where 1/world goes (the update's grad_scale).  All K passes are part of ONE captured graph / command list.

Averaged weights (`ema_decay=d`): an exponential moving average of every parameter and every BatchNorm running statistic lives in
one flat device buffer (ops.EmaTable) and is advanced at the end of the step, after Adam, by two launches that are part of the
captured / recorded step: `cris_ema_advance` decides on the device whether this optimizer step is an EMA step (`ema_every`) and
with which weight (`ema_warmup`), `cris_ema_update` applies ema += (p - ema) * weight to everything.  Once per optimizer step,
not per micro-batch; no communication (parameters, hence averages, are identical on every rank).  ema_state_dict() has the keys
of model_state_dict().  With ema_decay=None (the default) nothing is allocated and the step issues the launches it always did.

Per-step learning rates (`lr_schedule=table`): a float32 table [n_steps, 2] - row t = (backbone rate, rate of the rest) of 0-based
optimizer step t, steps past the end use the last row - lives on the device (ops.LrSchedule).  Immediately before the Adam launches
`cris_adam_schedule_lrs` (one launch per Adam table) copies the row of the running step, chosen from the device step counter, into
the `lr` fields of the Adam descriptors, where the Adam kernels read it: warm-up, cosine, one-cycle or any other per-iteration
schedule (cris.pytorch_amd.lr builds the tables) without host work and without a new capture.  Once per optimizer step, no
communication (every rank passes the same table).  With lr_schedule=None (the default) the step issues the launches it always did.

Weight decay (`weight_decay=w`, `decoupled_weight_decay`, `no_decay`): by default w is one scalar, applied as coupled L2 (g += w * p
before the moments) to every tensor, the reference's torch.optim.Adam.  `decoupled_weight_decay=True` makes it AdamW's
p *= 1 - lr * w on the weight itself, gradient and moments untouched, with the rate of the running step (the schedule's row when
there is one).  `no_decay` is a rule (name, tensor) -> bool that exempts tensors: no_decay_1d (biases, BatchNorm / LayerNorm scales
- what the reference's utils/misc.py:168-189 group_weight exempts) and no_decay_1d_and_positional (the positional embeddings too -
the `backbone_no_decay` group model/__init__.py:4-29 keeps commented out) are ready-made.  Either makes the Adam launches
`cris_adamw_step`, which reads one decay per tensor from a small device array: the same two launches, once per optimizer step,
independent of clipping (the norm is the raw gradient's), no communication.  With the defaults the step issues the launches it
always did - `cris_adam_step_amp` with the scalar - and nothing is allocated.

Loss (`loss=ops.SegLoss(...)`): bce_weight * BCE-with-logits(pos_weight) + dice_weight * soft Dice per sample, computed and
differentiated on the device by `cris_seg_loss_fwd` / `cris_seg_loss_bwd` in the place of `cris_bce_fwd` / `cris_bce_bwd`: two
forward launches and one backward launch, as before, inside the captured / recorded step.  The Dice term is a mean of per-sample
values, so it is exact under data parallelism and under accum_steps.  `loss_terms` holds the unweighted (bce, dice) of the step.
No communication; configuration like the schedule table, not part of optimizer_state_dict().  With loss=None (the default, and any
SegLoss equal to the defaults) the step issues the launches it always did and nothing is allocated.
"""
import contextlib
import os
from typing import Optional

import torch

from . import capture, debug, ops
from .arch import ClipSpec, HeadSpec
from .engine import Engine


def strip_ddp_prefix(sd):
    """The reference saves `model.state_dict()` of the DistributedDataParallel-wrapped model (train.py:192-204), so every key
    of its checkpoints starts with `module.`, and test.py:74-78 loads them strictly into a DataParallel wrapper.  Accept
    both spellings: a state_dict whose keys ALL carry the prefix is returned without it, anything else unchanged."""
    keys = list(sd.keys())
    if keys and all(k.startswith("module.") for k in keys):
        return {k[len("module."):]: v for k, v in sd.items()}
    return sd


def split_state_dict(sd, device):
    sd = strip_ddp_prefix(sd)
    params = {k: v.to(device).contiguous() for k, v in sd.items()
              if v.is_floating_point() and not k.endswith(("running_mean", "running_var"))}
    buffers = {k: v.to(device).contiguous() for k, v in sd.items() if k.endswith(("running_mean", "running_var"))}
    return params, buffers


def epoch_group_lrs(epoch, base_lr, lr_multi, milestones, gamma):
    """(lr_backbone, lr_head) the reference trains epoch `epoch` (0-based) with - train.py:105-110,210.
    Adam is built with lr=base_lr over groups that carry only `initial_lr`, so epoch 0 runs BOTH groups at base_lr;
    `scheduler.step(epoch_log)` with an explicit epoch then switches MultiStepLR to its closed form on `initial_lr`
    (= lr_multi*base_lr for the backbone group): lr_e = initial_lr * gamma ** #{m in milestones : m <= e} for e >= 1."""
    if epoch <= 0:
        return base_lr, base_lr
    f = gamma ** sum(1 for m in milestones if m <= epoch)
    return lr_multi * base_lr * f, base_lr * f


EMBEDDING = "backbone.token_embedding.weight"          # the tensor whose rows the update may skip (NativeTrainer.__init__)


def in_backbone_group(name):
    """`build_segmenter`'s name rule (model/__init__.py:36-48): group 0 = backbone without the positional embeddings, group 1 = the rest"""
    return name.startswith("backbone") and "positional_embedding" not in name


def no_decay_1d(name, tensor):
    """no_decay rule: every parameter with at most one dimension - biases and BatchNorm / LayerNorm scales, the `weight_decay=0`
    group of the reference's group_weight (utils/misc.py:168-189)"""
    return tensor.dim() <= 1


def no_decay_1d_and_positional(name, tensor):
    """no_decay rule: no_decay_1d plus the positional embeddings, the reference's commented-out `backbone_no_decay` group
    (model/__init__.py:4-29)"""
    return tensor.dim() <= 1 or "positional_embedding" in name


def checked_int(what, value, lowest):
    if isinstance(value, bool) or not isinstance(value, int) or value < lowest:
        raise ValueError("%s must be an integer >= %d, got %r" % (what, lowest, value))
    return value


class NativeTrainer:
    def __init__(self, clip: ClipSpec, head: HeadSpec, state_dict, device, base_lr=1e-4, lr_multi=0.1, weight_decay=0.0,
                 comm=None, sync_bn=False, use_graph: Optional[bool] = None, launch: Optional[str] = None, max_norm: float = 0.0,
                 track_grad_norm: bool = False, accum_steps: int = 1, ema_decay: Optional[float] = None, ema_every: int = 1,
                 ema_warmup: bool = False, lr_schedule=None, decoupled_weight_decay: bool = False, no_decay=None, loss=None):
        """loss = None: the reference's mean BCE with logits; an ops.SegLoss: weighted BCE + soft Dice on the device (the module
        docstring; set_loss; loss_terms).
        weight_decay = w >= 0: coupled L2 on every tensor (the reference's Adam); decoupled_weight_decay: AdamW's p *= 1 - lr * w
        instead; no_decay: None or a rule (name, tensor) -> bool, True = this tensor's decay is 0 (no_decay_1d,
        no_decay_1d_and_positional) - the module docstring; set_weight_decay; weight_decays.
        lr_schedule = array-like [n_steps, 2]: the (backbone, rest) learning rates of every optimizer step, followed on the device
        inside the captured step (the module docstring; set_lr_schedule; cris.pytorch_amd.lr builds such tables).
        ema_decay = d in (0, 1): keep an exponential moving average of parameters and BatchNorm statistics, updated every
        `ema_every`-th optimizer step with weight 1 - d (ema_warmup: 1 - min(d, (1 + t) / (10 + t)) for update t); set_ema.
        accum_steps = K > 1: one train_step is one optimizer step over K micro-batches (the module docstring; set_accum_steps).
        max_norm > 0: clip the gradients by their global 2-norm like the reference's `clip_grad_norm_(model.parameters(),
        args.max_norm)` (engine/engine.py:54-55); 0 (the shipped configs): no clipping.  track_grad_norm: compute `grad_norm`
        every step without clipping."""
        self.max_norm, self.track_grad_norm = self._checked_max_norm(max_norm), bool(track_grad_norm)
        self.accum_steps = checked_int("accum_steps", accum_steps, 1)
        ema_cfg = self._checked_ema(ema_decay, ema_every, ema_warmup)
        lr_schedule = self._checked_schedule(lr_schedule)
        decay_cfg = self._checked_weight_decay(weight_decay, decoupled_weight_decay, no_decay)
        loss = ops.SegLoss.normalized(loss)
        if no_decay is not None:                 # (the rule's answers are checked on the tensors as given, before a device is touched)
            self._exempt(no_decay, [(k, v) for k, v in strip_ddp_prefix(state_dict).items()
                                    if v.is_floating_point() and not k.endswith(("running_mean", "running_var"))])
        self.device = device
        params, buffers = split_state_dict(state_dict, device)
        self.engine = Engine(clip, head, params, buffers, device, comm=comm, sync_bn=sync_bn)
        self.comm = self.engine.comm
        e = self.engine
        if self.comm.world > 1:
            # DistributedDataParallel broadcasts rank 0's parameters and buffers when it wraps the module (train.py:100-102);
            # the single-exchange SyncBN takes its moments about the running mean, which must be bit-identical on every rank
            for t in list(e.P.values()) + list(e.Bf.values()):
                self.comm.broadcast(t, 0)
        self._checked_batch = None
        # `build_segmenter` groups: backbone (w/o positional embeddings) vs the rest.  torch's Adam is built with
        # lr=base_lr and groups that only carry `initial_lr`, so BOTH groups start at base_lr.
        names = [n for n in e.grad_order if n != "backbone.logit_scale"]          # never receives a gradient (unused)
        self.names = names
        self.group = {n: (0 if in_backbone_group(n) else 1) for n in names}
        self.base_lr, self.lr_multi = base_lr, lr_multi
        self.weight_decay, self.decoupled_weight_decay, self.no_decay = decay_cfg
        self._no_decay_names = self._exempt(no_decay, [(n, e.P[n]) for n in names])
        # Rows of the token embedding (49408 x 512: 17% of the parameters) that have never received a gradient keep g = m = v = 0
        # and Adam leaves them exactly as they are (while weight_decay == 0): the embedding backward marks the rows of each
        # batch's tokens and the update skips the rest - bit-identical to the dense update while the embedding's own decay is 0
        # (no weight decay at all, or the embedding exempt through `no_decay`).  With more ranks the all-reduced
        # gradient has the other ranks' rows too: the marks (sticky bytes) are then all-reduced with MAX next to the text
        # encoder's gradient stage (round 6; 49 KB per step on the gradient communicator), so every rank skips exactly the rows
        # no rank ever touched - communicators without a byte-wise MAX (dist.RcclComm) keep the dense update.
        # CRIS_ADAM_ROW_SKIP=0 switches it off.
        if ((self.comm.world == 1 or getattr(self.comm, "supports_max_u8", False)) and self.weight_decays[EMBEDDING] == 0.0
                and os.environ.get("CRIS_ADAM_ROW_SKIP", "1") == "1" and torch.device(device).type == "cuda"):
            e.embed_live = torch.zeros(e.P["backbone.token_embedding.weight"].shape[0], dtype=torch.uint8, device=device)
        self._build_adam([base_lr] * len(names))
        self._apply_weight_decay()
        self.metric = torch.zeros(2, device=device)
        # per-step device state: steps done (int32) and the dropout seed of the running step
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=device)
        self.seed_dev = torch.zeros(1, dtype=torch.int32, device=device)
        # generation of the peer-mailbox exchanges: advances with every step and is NEVER rewritten (the optimizer step is, by
        # load_optimizer_state_dict: a rewound generation would accept the stale words of its first use, csrc/p2p_ll.h)
        self.xgen_dev = torch.zeros(1, dtype=torch.int32, device=device)
        # SyncBN statistics: 142 exchanges of a few KB per step, all on the critical path.  Default: peer-mapped mailboxes, one
        # kernel per exchange (dist.PeerMailboxes) - when allocation, IPC mapping and a self-test with known data succeed on
        # EVERY rank; otherwise (and with CRIS_SYNCBN_P2P=0, or a communicator without mailboxes) the RCCL collectives.
        self.syncbn_exchange = "none" if not e.sync_bn else "collective"
        if (e.sync_bn and os.environ.get("CRIS_SYNCBN_P2P", "1") == "1"          # (world 1 + CRIS_FORCE_DIST: the exchange with itself)
                and torch.device(device).type == "cuda" and hasattr(self.comm, "enable_p2p")):
            cmax = max(e.P[pfx + ".weight"].numel() for pfx in e.bn_prefixes)
            why = self.comm.enable_p2p(slots=2 * len(e.bn_prefixes) + 8, max_floats=4 * cmax, gen_dev=self.xgen_dev)
            if why is None:
                fused = getattr(self.comm, "_fused", False)
                self.syncbn_exchange = "p2p mailboxes, exchanged inside the BatchNorm launches" if fused else "p2p mailboxes, one exchange kernel per BatchNorm"
            else:
                self.syncbn_exchange = "collective (mailboxes refused: %s)" % why
        # gradient exchange: RCCL through torch.distributed (the default: eight staged all-reduces on their own communicator and
        # stream); CRIS_GRAD_EXCHANGE=p2p: the direct reduce-scatter + all-gather over the peer-mapped gradient arenas
        # (dist.TorchDistComm.enable_arena_exchange) when mapping and self-test succeed on every rank, else RCCL
        self.grad_exchange = "none" if (self.comm.world == 1 and not debug.HOOKS.force_dist) else "rccl"
        if (os.environ.get("CRIS_GRAD_EXCHANGE", "rccl") == "p2p" and getattr(self.comm, "p2p", None) is not None
                and hasattr(self.comm, "enable_arena_exchange")):
            why = self.comm.enable_arena_exchange(e.grad_arena)
            self.grad_exchange = ("p2p: reduce-scatter + all-gather over the peer-mapped gradient arenas" if why is None
                                  else "rccl (arena exchange refused: %s)" % why)
        if launch is None:
            launch = os.environ.get("CRIS_LAUNCH")
        if launch is None:
            if use_graph is False or os.environ.get("CRIS_NO_GRAPH", "0") == "1":
                launch = "eager"
            else:
                # one captured HIP graph per step on any number of ranks: RCCL's kernels are captured like every other
                # launch (measured with a 1-rank RCCL group, tools/dist1_check.py: 15.4 ms/step captured against 16.9 as a
                # command list, ~145 collectives per step); a capture that fails on ANY rank makes every rank fall back
                # to the command list (train_step).  Communicators that cannot be captured (gloo: host copies) say so.
                launch = "graph" if getattr(self.comm, "capturable", True) else "cmdlist"
        if torch.device(device).type != "cuda":
            launch = "eager"
        assert launch in ("graph", "cmdlist", "eager"), launch
        self.launch = launch
        self.use_graph = launch != "eager"
        self._invalidate()
        self._static = None
        self.graph_error = None
        self._host_steps = 0
        self._acc = self._loss_acc = self._metric_micro = self._terms_acc = None
        self.set_accum_steps(self.accum_steps)
        self.set_loss(loss)
        self._ema = None
        self.set_ema(*ema_cfg)                   # (after the rank-0 broadcast above: the average starts from the shared values)
        self._lr = None
        self.set_lr_schedule(lr_schedule)
        self._peer_check_every = int(os.environ.get("CRIS_PEER_CHECK_EVERY", "200"))

    def _build_adam(self, lrs):
        e, names = self.engine, self.names
        lr_of = dict(zip(names, lrs))
        live = {names.index(EMBEDDING): e.embed_live} if e.embed_live is not None else None
        self.adam = ops.AdamTable([e.P[n] for n in names], [e.G[n] for n in names], [lr_of[n] for n in names],
                                  layouts=[e.gemm_layout(n) for n in names], packs=[e.pack_info.get(n) for n in names], row_live=live)

    def check_peer_timeout(self):
        """collective: raise on every rank if any rank's SyncBN mailbox exchange timed out (dist.TorchDistComm.check_peer_timeout)"""
        chk = getattr(self.comm, "check_peer_timeout", None)
        if chk is not None:
            chk()

    @property
    def step_idx(self):
        return int(self.step_dev.item())

    def set_group_lrs(self, lr_backbone, lr_head):
        """learning rates of the two groups from now on (host write + upload of the Adam tables; the step is captured / recorded
        again).  While a per-step schedule is on (set_lr_schedule) they last only until the next step, which overwrites them with
        its row of the table."""
        lrs = [lr_backbone if self.group[n] == 0 else lr_head for n in self.names]
        self.adam.set_lrs(lrs)
        self._invalidate()                       # learning rates live in the device table, which was re-uploaded (new address)

    def set_max_norm(self, max_norm):
        """change the clipping threshold (0 = off); it is an argument of a launch, so the step is captured / recorded again"""
        self.max_norm = self._checked_max_norm(max_norm)
        self._invalidate()

    @staticmethod
    def _checked_max_norm(max_norm):
        if not max_norm >= 0:
            raise ValueError("max_norm must be >= 0 (0 = no clipping), got %r" % (max_norm,))
        return float(max_norm)

    def _invalidate(self):
        """the captured graph / recorded list no longer describes the step: the next one runs eagerly, the one after it captures
        or records again"""
        self._graph = self._cmds = None
        self._eager_steps = 0

    def set_accum_steps(self, accum_steps):
        """number of micro-batches per optimizer step; the step is captured / recorded again.  K > 1 holds a second buffer of the
        gradient arena's size (the running sum), K == 1 holds none and runs exactly the step of a trainer without accumulation.
        The dropout seeds follow (step * K + micro) * 7919 + 17 with the K of the running step."""
        self.accum_steps = checked_int("accum_steps", accum_steps, 1)
        if self.accum_steps > 1:
            if self._acc is None:
                self._acc = torch.empty_like(self.engine.grad_arena)
                self._loss_acc = torch.zeros((), device=self.device)
                self._metric_micro = torch.zeros(2, device=self.device)
        else:
            self._acc = self._loss_acc = self._metric_micro = None
        self._size_terms_acc()
        self._invalidate()

    def set_loss(self, spec):
        """the loss from now on: None (or an ops.SegLoss equal to the defaults) = the reference's mean BCE with logits, else the
        ops.SegLoss (weighted BCE + soft Dice).  Its scalars are arguments of launches, so the step is captured / recorded again.
        Configuration, like the schedule table: not written into optimizer_state_dict() and not restored."""
        self.engine.set_loss(spec)
        self._size_terms_acc()
        self._invalidate()

    def _size_terms_acc(self):
        """the running mean of the micro-batches' loss terms: held only with a SegLoss AND accum_steps > 1"""
        if self.engine.loss_spec is not None and self.accum_steps > 1:
            if self._terms_acc is None:
                self._terms_acc = torch.zeros(2, device=self.device)
        else:
            self._terms_acc = None

    @property
    def loss_spec(self):
        return self.engine.loss_spec

    @property
    def loss_terms(self):
        """the unweighted (bce, dice) of the last step under a SegLoss: a device tensor [2] written by the step itself (no sync
        here), overwritten by the next step; with accum_steps = K > 1 the mean over the K micro-batches.  None with the default
        loss, and before the first step."""
        if self.engine.loss_spec is None:
            return None
        return self._terms_acc if self.accum_steps > 1 else self.engine.loss_terms

    @staticmethod
    def _checked_ema(decay, every, warmup):
        if decay is not None and (isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 < decay < 1.0):
            raise ValueError("ema_decay must be None (off) or a number in (0, 1), got %r" % (decay,))
        return (None if decay is None else float(decay)), checked_int("ema_every", every, 1), bool(warmup)

    def set_ema(self, decay, every=1, warmup=False):
        """switch the weight average on (0 < decay < 1), change its settings, or switch it off (None: the buffer is freed); the
        step is captured / recorded again.  Switching it ON sets the average to the current parameters and BatchNorm statistics
        and its update count to 0; changing decay / every / warmup of a running average keeps both.  Costs one more fp32 copy
        of the parameters and buffers."""
        self.ema_decay, self.ema_every, self.ema_warmup = self._checked_ema(decay, every, warmup)
        if self.ema_decay is None:
            self._ema = None
        elif self._ema is None:
            e = self.engine
            skip = e.embed_live is not None and self.weight_decays[EMBEDDING] == 0.0      # (a decayed row moves without a gradient)
            self._ema = ops.EmaTable(list(e.P.items()) + list(e.Bf.items()), row_live={EMBEDDING: e.embed_live} if skip else None)
            self._ema.reset()
        self._invalidate()

    @staticmethod
    def _checked_weight_decay(weight_decay, decoupled, no_decay):
        """(weight_decay as a float, decoupled as a bool, no_decay), or ValueError"""
        if no_decay is not None and not callable(no_decay):
            raise ValueError("no_decay must be None or a callable (name, tensor) -> bool, got %r" % (no_decay,))
        return ops.AdamTable.checked_decay("weight_decay", weight_decay), bool(decoupled), no_decay

    @staticmethod
    def _exempt(no_decay, named):
        """names of the (name, tensor) pairs the rule exempts from weight decay; ValueError for an answer that is not a bool"""
        out = set()
        if no_decay is None:
            return out
        for n, t in named:
            r = no_decay(n, t)
            if not isinstance(r, bool):
                raise ValueError("no_decay(%r, tensor) must return a bool, got %r" % (n, r))
            if r:
                out.add(n)
        return out

    @property
    def weight_decays(self):
        """{name: the weight decay tensor `name` is updated with}: weight_decay, or 0 where `no_decay` exempts it"""
        return {n: (0.0 if n in self._no_decay_names else self.weight_decay) for n in self.names}

    def _apply_weight_decay(self):
        """one decay per tensor in the Adam tables (cris_adamw_step) when the decay is decoupled or some tensor is exempt; else the
        scalar of cris_adam_step_amp, as always"""
        per_tensor = self.decoupled_weight_decay or bool(self._no_decay_names)
        wd = self.weight_decays
        self.adam.set_decay([wd[n] for n in self.names] if per_tensor else None, self.decoupled_weight_decay)

    def set_weight_decay(self, weight_decay, decoupled=False, no_decay=None):
        """change the weight decay, whether it is decoupled and which tensors are exempt (all three: the constructor's arguments);
        the step is captured / recorded again.  The marks of the token-embedding row skip are allocated by the constructor only
        (when the embedding's own decay is 0 there); when the embedding becomes decayed the update ignores them (its rows move
        without a gradient), and a running weight average stops skipping rows for good."""
        cfg = self._checked_weight_decay(weight_decay, decoupled, no_decay)
        exempt = self._exempt(no_decay, [(n, self.engine.P[n]) for n in self.names])
        (self.weight_decay, self.decoupled_weight_decay, self.no_decay), self._no_decay_names = cfg, exempt
        self._apply_weight_decay()
        if self._ema is not None and self.weight_decays[EMBEDDING] != 0.0:
            self._ema.drop_row_live()
        self._invalidate()

    @staticmethod
    def _checked_schedule(table):
        """None, or the table as float32 numpy [n_steps, 2] (converted once); ValueError for anything else"""
        if table is None:
            return None
        try:
            return ops.LrSchedule.checked_table(table, n_groups=2)
        except ValueError as ex:
            raise ValueError("lr_schedule: %s" % ex)

    def set_lr_schedule(self, table):
        """switch the per-step learning rates on or replace them (array-like [n_steps, 2]: column 0 the backbone group, column 1
        the rest; row t = the rates of 0-based optimizer step t, steps past the end use the last row), or switch them off (None:
        the device buffers are freed and the rates set last through set_group_lrs / set_epoch / the constructor hold again).  The
        step is captured / recorded again.  The row is chosen from the optimizer step count, which load_optimizer_state_dict
        restores: a resumed run continues at the right row once the same table has been set; the table itself is configuration
        and not part of optimizer_state_dict().  As with torch, a state saved under a schedule carries the next row's rates as the
        groups' `lr`, and load_optimizer_state_dict makes them the host's rates (set_group_lrs): on a resumed trainer those, not
        the constructor's, are what None goes back to - call set_group_lrs / set_epoch after switching off to choose others."""
        table = self._checked_schedule(table)
        if table is None:
            if self._lr is not None:
                self._lr = None
                self.adam.set_lrs(self.adam.lrs)         # the device tables hold the last row: back to the host's rates
        else:
            self._lr = ops.LrSchedule(self.adam, [self.group[n] for n in self.names], table, checked=True)
        self._invalidate()

    @property
    def current_lrs(self):
        """(backbone rate, rate of the rest) the last step used: a device tensor [2] written by the step itself (no sync here),
        overwritten by the next step; zeros before the first one.  Only with a per-step schedule."""
        if self._lr is None:
            raise RuntimeError("current_lrs is written only with a per-step schedule: pass lr_schedule or call set_lr_schedule(table)")
        return self._lr.lr_out

    def _ema_table(self):
        if self._ema is None:
            raise RuntimeError("no weight average is kept: build the trainer with ema_decay or call set_ema(decay)")
        return self._ema

    @property
    def ema_num_updates(self):
        """EMA updates applied so far (selects the warm-up weight of the next one); reads the device counter"""
        return self._ema_table().num_updates

    @property
    def grad_norm(self):
        """2-norm of the last step's (rank- and micro-batch-averaged, unclipped) gradient: a 0-dim device tensor, overwritten by the next step.
        Only computed when max_norm > 0 or track_grad_norm is set."""
        if not (self.max_norm > 0 or self.track_grad_norm):
            raise RuntimeError("grad_norm is computed only with max_norm > 0 or track_grad_norm=True")
        return self.adam.gnorm[0]

    def set_epoch(self, epoch, milestones=(35,), gamma=0.1):
        """Learning rates of the reference schedule for `epoch` (0-based); call at every epoch boundary.  While a per-step schedule
        is on (set_lr_schedule) the next step overwrites them with its row of the table: use one or the other
        (lr.reference_epochs is this recipe as a table)."""
        self.set_group_lrs(*epoch_group_lrs(epoch, self.base_lr, self.lr_multi, milestones, gamma))

    # ------------------------------------------------------------------------------------------------
    def _step_body(self, img, word, mask, host_seed: Optional[int]):
        """the step over K = accum_steps micro-batches (views of the inputs' K equal slices; the module docstring).  K == 1 is the
        plain step: no running sums, the metric written straight into self.metric, the engine's own loss returned"""
        e, K = self.engine, self.accum_steps
        b = img.shape[0] // K
        if K > 1:
            ops.zero_(self._loss_acc)
            ops.zero_(self.metric)
            if self._terms_acc is not None:
                ops.zero_(self._terms_acc)
        for m in range(K):
            if K == 1:
                ops.step_advance(self.step_dev, self.seed_dev, self.xgen_dev)
            else:
                # the step counter advances with micro-batch 0, the seed and the mailbox generation with every micro-batch
                ops.step_advance_micro(self.step_dev, self.seed_dev, self.xgen_dev, m, K)
            if host_seed is None:
                e.seed_dev, seed = self.seed_dev, 0
            else:                                # explicit seed (tests): a host value, seed + m for micro-batch m; the device
                e.seed_dev, seed = None, host_seed + m                                        # counter still advances
            micro = (img, word, mask) if K == 1 else [x[m * b:(m + 1) * b] for x in (img, word, mask)]
            pred, msk, loss = e.forward(*micro, training=True, seed=seed)
            if K > 1:
                ops.axpy_f32(self._loss_acc, loss, 1.0 / K)
                if self._terms_acc is not None:
                    ops.axpy_f32(self._terms_acc, e.loss_terms, 1.0 / K)
            self._metric(pred, msk)
            e.backward(on_stage_done=self._stage_hook(m))
        if self._exchanges():
            ops.torch_op(self.comm.wait_all)
        self._update(1.0 / (self.comm.world * K))            # the 1/K goes where 1/world goes
        return (loss if K == 1 else self._loss_acc), pred, msk

    def _exchanges(self):
        return self.comm.world > 1 or debug.HOOKS.force_dist

    def _metric(self, pred, msk):
        """the train metric (utils/misc.py:114-129) only needs the logits: it runs on the text-encoder stream underneath the
        backward pass (backward() joins that stream before it returns).  K > 1: the mean of the micro-batches' metrics, which is
        the whole batch's (equal sizes)"""
        e, K = self.engine, self.accum_steps
        if e.side is not None:
            cur = torch.cuda.current_stream()
            ops.torch_op(lambda: e.side.wait_stream(cur))
        with (torch.cuda.stream(e.side) if e.side is not None else contextlib.nullcontext()):
            ops.train_metric(pred, msk, pred.shape[0], pred.shape[2] * pred.shape[3], self.metric if K == 1 else self._metric_micro)
            if K > 1:
                ops.axpy_f32(self.metric, self._metric_micro, 1.0 / K)

    def _stage_hook(self, m):
        """backward's stage hook of micro-batch m, or None when there is neither a sum to keep nor an exchange to start.  It fires on
        the stream the stage's gradients were issued on (stage 4: the side stream)"""
        e, K, exchange = self.engine, self.accum_steps, self._exchanges()
        if K == 1 and not exchange:
            return None
        last = m == K - 1

        def on_stage(st):
            lo, hi = e.stage_ranges[st]
            g = e.grad_arena[lo:hi]
            if K > 1:
                acc = self._acc[lo:hi]
                if not last:
                    ops.grad_accumulate(acc, g, add=m > 0)       # acc = g0 ; acc += g_m
                    return
                ops.grad_accumulate(g, acc)                      # the total, in the arena, before the stage's exchange
            if exchange:
                self._exchange_stage(st, g)
        return on_stage

    def _exchange_stage(self, st, g):
        ops.torch_op(lambda: self.comm.allreduce_async(g))
        if st == 4 and self.engine.embed_live is not None and getattr(self.comm, "supports_max_u8", False):
            # (stage 4 = the text encoder, whose backward marked the rows of the token embedding; the marks are sticky: the rows
            # of every micro-batch of this step, and of every step before)
            ops.torch_op(lambda: self.comm.allreduce_async(self.engine.embed_live, op="max"))

    def _update(self, grad_scale):
        """the tail of the step, once per optimizer step: norm / divisor, schedule row, one Adam pass over every tensor (it also
        rewrites the bf16 operand copies of the GEMM weights from the new values), EMA"""
        divisor = None
        if self.max_norm > 0 or self.track_grad_norm:
            # clip_grad_norm_ (engine/engine.py:54-55) as a divisor of the update: the norm of the averaged gradient and
            # max(1, norm / max_norm) are left on the device, the Adam kernels divide by it where GradScaler's scale goes
            gn = self.adam.grad_norm(grad_scale=grad_scale, max_norm=self.max_norm if self.max_norm > 0 else None)
            if self.max_norm > 0:
                divisor = gn[1:2]
        if self._lr is not None:                 # the row of step_dev, which micro-batch 0 advanced
            self._lr.apply(self.step_dev)
        self.adam.step(weight_decay=0.0 if self.adam.decays is not None else self.weight_decay, grad_scale=grad_scale,
                       step_dev=self.step_dev, loss_scale_dev=divisor)
        self.engine.packs_current = self.adam.refreshes_packs
        if self._ema is not None:
            self._ema.update(self.step_dev, self.ema_every, self.ema_decay, self.ema_warmup)

    def train_step(self, img, word, mask, seed: Optional[int] = None):
        """One optimizer step.  Returns (loss 0-dim device tensor, metric [IoU%, Pr@50%] device tensor); both are
        overwritten by the next call.  With accum_steps = K > 1 the inputs hold the whole optimizer batch of K * b samples,
        micro-batch m is samples [m*b, (m+1)*b), and loss and metric are the means over the K micro-batches."""
        if img.shape[0] % self.accum_steps:
            raise ValueError("batch of %d samples is not a multiple of accum_steps = %d" % (img.shape[0], self.accum_steps))
        # COLLECTIVE, every CRIS_PEER_CHECK_EVERY-th step (default 200; 0 = never): a rank whose SyncBN mailbox exchange gave up
        # waiting for a peer raises on EVERY rank instead of training on alone (round-5 advisor finding: nothing called the check)
        self._host_steps += 1
        if self._peer_check_every > 0 and self._host_steps % self._peer_check_every == 0 and getattr(self.comm, "p2p", None) is not None:
            self.check_peer_timeout()
        self._check_equal_batch(img.shape[0])
        if not self.use_graph or seed is not None or ops.KERNEL_TIMER is not None:
            loss, _, _ = self._step_body(img, word, mask, seed)
            return loss, self.metric
        key = (tuple(img.shape), tuple(word.shape), tuple(mask.shape))
        if self._static is not None and self._static[0] != key:
            self._invalidate()                   # new shapes: new schedule
            self._static = None
        self._static = (key, capture.stage(self._static and self._static[1], (img, word, mask), self.device))
        if self._graph is None and self._cmds is None:
            def body():
                return self._step_body(*self._static[1], None)
            if self._eager_steps < 1:
                # first step with these shapes runs eagerly: constant tables get uploaded, the allocator warms up
                self._eager_steps += 1
                return body()[0], self.metric
            if self.launch == "graph":
                err = None
                try:
                    # (capture.py: thread_local mode + a drained c10d watchdog - the eager first step left collectives of
                    # two communicators behind whose end events the watchdog thread is still polling)
                    self._graph, (self._loss, *self._keep) = capture.build("graph", body, device=self.device)
                except Exception as ex:          # noqa: BLE001 - e.g. a collective that cannot be captured
                    err = repr(ex)
                if self.comm.world > 1:          # the ranks must agree on the launch mode
                    err = next((x for x in self.comm.all_gather_object(err) if x), None)
                if err is not None:
                    self.graph_error, self._graph = err, None
                    torch.cuda.synchronize(self.device)
                    self.launch = "cmdlist" if self.comm.world > 1 else "eager"
                    self.use_graph = self.launch == "cmdlist"
            if self.launch == "eager":
                return body()[0], self.metric
            if self.launch == "cmdlist":
                # this call executes the step while recording it; its buffers come from the list's own MemPool
                self._cmds, (self._loss, *self._keep) = capture.build("cmdlist", body)
                return self._loss, self.metric
        (self._graph if self._graph is not None else self._cmds).replay()
        return self._loss, self.metric

    def _check_equal_batch(self, b):
        """SyncBN's global count is local count x world: every rank must feed the same per-rank batch (the reference's
        DistributedSampler + fixed DataLoader batch size guarantee it; checked once per batch size, not per step)."""
        if self.comm.world > 1 and self._checked_batch != b:
            sizes = self.comm.all_gather_object(int(b))
            if any(x != sizes[0] for x in sizes):
                raise ValueError("per-rank batch sizes differ across ranks (%s): SyncBN statistics assume equal shards" % (sizes,))
            self._checked_batch = b

    # ------------------------------------------------------------------------------------------------
    # checkpointing (reference train.py:159-174,192-207: {'epoch', 'cur_iou', 'best_iou', 'state_dict', 'optimizer', 'scheduler'})
    # ------------------------------------------------------------------------------------------------
    def _param_order(self):
        """parameter names in the order torch.optim.Adam(param_list) numbers them for `build_segmenter`'s two groups
        (model/__init__.py:36-48): group 0 = backbone without the positional embeddings, group 1 = the rest - module order
        inside each group.  `backbone.logit_scale` is a parameter of the reference module too (it just never gets a gradient)."""
        names = list(self.engine.P.keys())                    # state_dict (= named_parameters) order
        return [n for n in names if in_backbone_group(n)], [n for n in names if not in_backbone_group(n)]

    def model_state_dict(self, ddp_prefix=False):
        """the reference module's `state_dict()` (parameters + BatchNorm buffers; clones, on the CPU).  `ddp_prefix=True`:
        keys spelled `module.<name>` like the checkpoints the reference writes from its DDP-wrapped model
        (train.py:192-204) - what its `--resume` (train.py:159-174) and test.py:74-78 load strictly.
        `num_batches_tracked` counts forward passes, step_idx * accum_steps: exact only while accum_steps has not changed
        during the run."""
        e = self.engine
        return self._state_dict_of({k: v for k, v in list(e.P.items()) + list(e.Bf.items())}, ddp_prefix)

    def ema_state_dict(self, ddp_prefix=False):
        """the averaged weights in the form of model_state_dict(): same keys, same order, loadable wherever that one is
        (InferenceRunner.load_state_dict, the reference's test.py); `num_batches_tracked` is the live model's"""
        return self._state_dict_of(self._ema_table().views, ddp_prefix)

    def _state_dict_of(self, tensors, ddp_prefix):
        e = self.engine
        out = {k: v.detach().cpu().clone() for k, v in tensors.items()}
        steps = self.step_idx * self.accum_steps         # forward passes (exact while accum_steps has not changed during the run)
        for pfx in e.bn_prefixes:
            out[pfx + ".num_batches_tracked"] = torch.tensor(steps, dtype=torch.int64)
        # reference key order (module order), not "parameters then buffers"
        from .arch import build_param_tree
        order = list(build_param_tree(e.clip, e.head).state_dict().keys())
        assert set(order) == set(out.keys())
        out = {k: out[k] for k in order}
        if ddp_prefix:
            out = {"module." + k: v for k, v in out.items()}
        return out

    def _load_named(self, targets, sd):
        """copy sd[name] into every tensor of `targets` {name: tensor}; sd's keys may all carry DDP's `module.` prefix"""
        sd = strip_ddp_prefix(sd)
        missing = [k for k in targets if k not in sd]
        if missing:
            raise KeyError("state_dict lacks %d keys, e.g. %s" % (len(missing), missing[:3]))
        for k, t in targets.items():
            t.copy_(sd[k].to(self.device))

    def load_model_state_dict(self, sd):
        """parameters and BatchNorm buffers from a reference-keyed state_dict; the bf16 operand copies are re-packed on the
        next forward.  Keys may carry DDP's `module.` prefix (reference checkpoints do)."""
        e = self.engine
        self._load_named({**e.P, **e.Bf}, sd)
        e.packs_current = False
        if self._ema is not None:                # the average restarts from the loaded weights (load_ema_state_dict overrides)
            self._ema.reset()

    def load_ema_state_dict(self, sd, num_updates):
        """restore the averaged weights (ema_state_dict(); keys may carry `module.`) and the update count (ema_num_updates).
        When resuming, call it after load_model_state_dict, which resets the average to the loaded weights."""
        ema, e = self._ema_table(), self.engine
        checked_int("num_updates", num_updates, 0)
        self._load_named(ema.views, sd)
        ema.state.copy_(torch.tensor([num_updates, 0, 0, 0], dtype=torch.int32))
        # the update skips embedding rows that never had a gradient because there ema == p; an average from elsewhere may differ
        # from the parameters in such a row, and the skip would freeze that difference: then every row is updated from now on
        for name, live in list(ema.row_live.items()):
            dead = live == 0
            if bool((ema.views[name][dead] != e.P[name][dead]).any()):
                ema.drop_row_live()
                break

    def optimizer_state_dict(self):
        """Adam state in torch.optim.Adam.state_dict() form, loadable by the optimizer `train.py:105-107` builds from
        `build_segmenter`'s param_list (and by load_optimizer_state_dict).  With a per-step schedule the groups' `lr` is the row
        the NEXT step will use (as torch reports it after scheduler.step()); the table itself is not saved.  With decoupled decay
        both groups carry `decoupled_weight_decay: True` (torch.optim.Adam's own key), with exempt tensors each group carries
        `no_decay_params`, the indices of its exempt parameters; with the defaults neither key exists."""
        g0, g1 = self._param_order()
        idx = {n: i for i, n in enumerate(self.names)}
        lr_of = dict(zip(self.names, self.adam.lrs))
        state, step = {}, self.step_idx
        if self._lr is not None:
            row = [float(x) for x in self._lr.at(step)]
            lr_of = {n: row[self.group[n]] for n in self.names}
        for i, n in enumerate(g0 + g1):
            if n in idx and step > 0:
                j = idx[n]
                state[i] = {"step": torch.tensor(float(step)), "exp_avg": self.adam.m[j].detach().cpu().clone(),
                            "exp_avg_sq": self.adam.v[j].detach().cpu().clone()}
        def group(names, initial_lr, first):
            lr = next((lr_of[n] for n in names if n in lr_of), self.base_lr)
            g = {"lr": lr, "initial_lr": initial_lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": self.weight_decay,
                 "amsgrad": False, "params": list(range(first, first + len(names)))}
            if self.decoupled_weight_decay:
                g["decoupled_weight_decay"] = True
            if self._no_decay_names:
                g["no_decay_params"] = [first + i for i, n in enumerate(names) if n in self._no_decay_names]
            return g
        return {"state": state, "param_groups": [group(g0, self.lr_multi * self.base_lr, 0), group(g1, self.base_lr, len(g0))]}

    def load_optimizer_state_dict(self, sd):
        """restore m / v / step count (and the group learning rates) from optimizer_state_dict() or from the state_dict of a
        torch.optim.Adam over the same param_list.  The groups' `lr` become the host's rates through set_group_lrs; a state saved
        under a per-step schedule holds a row of its table there (set_lr_schedule).  The weight-decay settings (`weight_decay`,
        `decoupled_weight_decay`, `no_decay_params`) are configuration like the schedule table and are NOT restored: they stay
        what the constructor or set_weight_decay made them."""
        g0, g1 = self._param_order()
        idx = {n: i for i, n in enumerate(self.names)}
        step = 0
        for i, n in enumerate(g0 + g1):
            st = sd["state"].get(i)
            if st is None or n not in idx:
                continue
            j = idx[n]
            self.adam.m[j].copy_(st["exp_avg"].to(self.device))
            self.adam.v[j].copy_(st["exp_avg_sq"].to(self.device))
            step = max(step, int(float(st["step"])))
        for j, live in self.adam.row_live.items():       # rows with Adam state are live rows
            live.copy_(((self.adam.m[j] != 0) | (self.adam.v[j] != 0)).any(dim=1))
        self.step_dev.fill_(step)
        self.adam.step_count = step
        self.set_group_lrs(sd["param_groups"][0]["lr"], sd["param_groups"][1]["lr"])

    @torch.no_grad()
    def eval_forward(self, img, word):
        return self.engine.forward(img, word, None, training=False)
