"""MUNIT_Trainer: drop-in for the reference's scripts/trainer.py hot path on MI355X.

Same constructor / gen_update / dis_update / update_learning_rate / forward / sample / save /
resume surface and `self.loss_*` attribute names, so scripts/train.py
can swap `from trainer import MUNIT_Trainer` for `from munit_amd.trainer import MUNIT_Trainer`.

What is different underneath (none of it changes results beyond fp32 rounding):
  * every layer runs as a HIP kernel (munit_amd.ops); nothing falls back to torch ops;
  * generator and discriminator parameters, their gradients and the Adam moments live in flat
    fp32 buffers: backward-weight accumulates straight into the flat gradient, Adam is one
    fused kernel per optimizer, and data-parallel training is ONE all-reduce per update over
    RCCL/xGMI (torch.distributed backend "nccl") of that flat buffer -- 109 MB (G) / 66 MB (D);
  * work the reference does and then throws away is skipped: D weight-gradients inside
    gen_update (zeroed by dis_update, trainer.py:1145), the autograd graph of the generator
    inside dis_update (x_ba / x_ab are detached at trainer.py:1178-1179);
  * loss scalars stay on the device; nothing synchronises the host inside an update.

The semantic-consistency loss (semantic_w > 0 with a semantic_ckpt_path) runs the user's frozen Resnet34_8s on
the device (munit_amd/segmentation.py).  The synthetic-pair iteration of scripts/train.py:229-260 --
gen_update(..., synth=True, semantic_gt_a, semantic_gt_b) -- adds the pair reconstruction loss (recon_synth_w) and takes
the semantic loss against the simulator's label maps, the 19 logits merged into 10 classes inside the head kernel; the
pairs, masks and label maps come in as tensors, as munit_amd.data.get_synthetic_data_loader yields them.

Feature-level domain adaptation (adaptation.dfeat_lambda > 0, trainer.py:161-179): two domainClassifier(256) networks on the
content codes, trained by domain_classifier_sr_update (training-mode BatchNorm2d, max-pool and 16x16 average are HIP kernels
of their own, dann.hip) under their own optimizer classif_opt_sr; adaptation.adv_lambda > 0 adds the fooling term
(target 0.5) to gen_update, whose backward forms the gradient of the two content codes only -- the classifiers' weight
gradients, which the reference computes and zeroes unused (trainer.py:1241), are skipped.  fp32 only; like the reference,
save / resume do not carry the classifiers.

Output-level domain adaptation (adaptation.output_classifier_lambda > 0 and adaptation.output_adv_lambda > 0,
trainer.py:181-201): two more MsImageDis, output_classifier_sr_a / _b, on the images themselves, trained by
output_domain_classifier_sr_update (simulated -> 0, real -> 1) under their own optimizer output_classif_opt_sr, which takes
the plain step() as the reference's update does; gen_update adds calc_gen_loss_sr (target 0.5) of the two translations
with weight output_adv_lambda, forming no classifier weight gradient (the next update's zero_grad would discard it).  The
multi-scale loss of a discriminator pass is one kernel pair (ops.lsgan_loss).  dis.gan_type: nsgan (the discriminators'
non-saturating loss, ops.nsgan_loss inside MsImageDis) needs no code here; together with output_adv_lambda > 0 it is refused,
since the fooling term is calc_gen_loss_sr, whose nsgan branch raises NameError in the reference.  Either weight without the
other is refused; fp32, Adam only.  As in the reference, update_learning_rate does not step output_scheduler_sr and save / resume do not carry
these classifiers either.

Both adaptation levels train data-parallel under the build extension adaptation.data_parallel: 1 (default 0: a process
group of more than one rank is refused, as a change of the batch statistics should be a visible decision).  The two
classifier updates all-reduce their optimizers' flat gradients in line before the step, and the feature classifiers'
training-mode batch norms take their statistics over all ranks, forward and backward, in the classifier update and in
gen_update's fooling term (ops.bn_world, munit_batchnorm_dp_*): W ranks on W equal part-batches compute what one process
computes on the joined batch, and all ranks end every update with bitwise identical weights and running statistics.  The
output classifiers have no batch statistics; their fooling term lands in the generator's flat gradient and needs no
exchange of its own.

The segmentation head (adaptation.sem_seg_lambda > 0 with a semantic_ckpt_path, trainer.py:203-223 and 1286-1324): the
checkpoint's layer4, the 7x7 average and a fresh Conv2d(512, 10, 1) on the content codes (segmentation.SegmentationHead),
trained by segmentation_head_update against the simulator's label maps under its own optimizer segmentation_opt -- two
forwards of the head, a then b, each with its own batch statistics, the bilinear up-sample inside the cross-entropy kernel,
the plain step().  The encoders run without a tape there: the reference back-propagates into them, but gen_update zeroes
that gradient before any use.  fp32, Adam and one process only; update_learning_rate does not step scheduler_seg and
save / resume do not carry the head, as in the reference.

The domain-invariant perceptual loss (vgg_w > 0 with a vgg_model_path, trainer.py:493-502 and 618-636): the frozen VGG16
of munit_amd/vgg.py, read from <vgg_model_path>/models/vgg16.weight -- the cache file of the reference's load_vgg16, whose
download-and-convert step cannot run any more; the user supplies the file.  gen_update runs the two translations through
the network as one batch of 2B with gradient and the two originals as one batch of 2B without, and takes
mean((IN(f) - IN(t))^2) of relu5_3 per pair in one kernel pair (ops.in_mse); self.instancenorm stays the parameter-free
attribute the reference has, and the network is kept out of state_dict().  fp32 only, crops of at least 16x16.

With that every live branch of scripts/train.py's loop runs here.  The one weight still refused, domain_adv_w, cannot run
in the reference either (the a/b domain classifier's loss builds a 4-element target for any batch and save / resume read
an attribute that does not exist); vgg_w without a vgg_model_path is refused because the reference's load_vgg16 is dead.
"""
import os
import warnings

import torch
import torch.nn as nn
from torch.optim import Optimizer

from . import ops
from .networks import (AdaINGen, AdaINGen_double, ContentEncoder, InstanceNorm2d, MsImageDis, _ApplyRefreshesImages,
                       domainClassifier)
from .segmentation import SegmentationHead, colorize, load_segmentation_head, seg_head_loss, seg_loss
from .utils import get_model_list, get_scheduler, load_segmentation_model, normalize_config, weights_init
from .vgg import check_hw as check_vgg_hw, load_vgg16, vgg_loss


class StepGate:
    """An optimizer step that is still in flight on another stream (FusedAdam.step_on), and who has waited for it.
    `pending` is the event recorded behind the step, or None; `waited` the handles of the streams already ordered behind it;
    `device` the device both belong to.  The gate refers to no trainer, optimizer, module or tensor, so the modules that
    consult it (MsImageDis) can be copied without dragging any of those along: a copy gets a fresh, idle gate."""

    def __init__(self):
        self.pending, self.waited, self.device = None, set(), None
        self.event = None                     # recorded anew by every deferred step; dropped when the optimizer is re-bound

    def arm(self, event, device=None):
        self.event = self.pending = event
        self.waited, self.device = set(), device

    def wait(self, *_):
        """Order the current stream behind the pending step (no-op when none is pending, or when this stream has waited:
        every stream that reaches the weights waits once)."""
        ev = self.pending
        if ev is None:
            return
        st = torch.cuda.current_stream(self.device)
        if st.cuda_stream not in self.waited:
            st.wait_event(ev)
            self.waited.add(st.cuda_stream)

    def settle(self, *_):
        """A host-side reader or writer of the optimizer's buffers is about to start: the current stream waits, nothing pends."""
        if self.pending is not None:
            self.wait()
            self.pending, self.waited = None, set()

    def reset(self):
        self.settle()
        self.event = self.device = None

    def __deepcopy__(self, memo):
        return StepGate()


class FusedAdam(Optimizer):
    """torch.optim.Adam semantics (L2-coupled weight decay, amsgrad off; trainer.py:109-120)
    executed as one HIP kernel over a flat parameter buffer.  state_dict()/load_state_dict()
    speak torch.optim.Adam's format so `optimizer.pt` files interchange with the reference.

    `gate` (StepGate) orders everything behind a step that step_on() left in flight on another stream: every method below that
    reads or writes the flat buffers settles it first (one attribute test while nothing is pending), and the modules whose
    parameters live here consult it (MsImageDis.follow, _ApplyRefreshesImages).  Only code that reads flat_p / flat_g /
    flat_m / flat_v directly calls settle() itself."""

    def __init__(self, params, lr, betas, weight_decay, eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False))
        self._plist = [p for g in self.param_groups for p in g["params"]]
        self._step = 0
        self.flat_p = self.flat_g = self.flat_m = self.flat_v = None
        self._views = None
        self.gate = StepGate()
        # prepared weight images (ops._prepared): items registered on first use, refreshed in one launch per step
        self._prep_items = []
        self._prep_table = None

    # ---- flat storage -----------------------------------------------------------------
    @staticmethod
    def _view(flat, off, p):
        n = p.numel()
        v = flat[off:off + n]
        if p.dim() == 4:
            o, i, kh, kw = p.shape
            return v.view(o, kh, kw, i).permute(0, 3, 1, 2)  # logical OIHW, memory [O][KH][KW][I]
        return v.view(p.shape)

    def bind(self, device):
        """(Re)build the flat buffers on `device`, re-pointing every parameter at its slice."""
        self.gate.reset()                     # the old buffers are read below; the event belonged to their device
        offs, total = [], 0
        for p in self._plist:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4  # keep every tensor 16-byte aligned
        flat_p = torch.zeros(total, dtype=torch.float32, device=device)
        flat_g = torch.zeros(total, dtype=torch.float32, device=device)
        flat_m = torch.zeros(total, dtype=torch.float32, device=device)
        flat_v = torch.zeros(total, dtype=torch.float32, device=device)
        if self.flat_m is not None and self.flat_m.numel() == total:
            flat_m.copy_(self.flat_m)
            flat_v.copy_(self.flat_v)
        views = []
        with torch.no_grad():
            for p, off in zip(self._plist, offs):
                if p.dtype != torch.float32:
                    raise RuntimeError("munit_amd: parameters must stay float32")
                pv = self._view(flat_p, off, p)
                pv.copy_(p.data)
                p.data = pv
                gv = self._view(flat_g, off, p)
                p._munit_grad = gv
                p.grad = gv
                p._munit_prep = {}       # the storage moved: every prepared image is void
                p._munit_opt = self
                views.append((self._view(flat_m, off, p), self._view(flat_v, off, p)))
        self.flat_p, self.flat_g, self.flat_m, self.flat_v = flat_p, flat_g, flat_m, flat_v
        self._views = views
        self._offsets = offs                  # start of every parameter in the flat buffers (16-byte aligned slots)
        self._total = total
        self._prep_items, self._prep_table = [], None

    def ranges_of(self, select):
        """Maximal contiguous [start, end) element ranges of the flat buffers covered by the parameters p with
        select(p) true, in buffer order (alignment gaps between two selected parameters belong to the range)."""
        out = []
        ends = self._offsets[1:] + [self._total]
        for p, a, b in zip(self._plist, self._offsets, ends):
            if not select(p):
                continue
            if out and out[-1][1] == a:
                out[-1][1] = b
            else:
                out.append([a, b])
        return [tuple(r) for r in out]

    # ---- prepared weight images ----------------------------------------------------------
    def register_prepared(self, item):
        """Called by ops._prepared the first time a layer needs a re-laid-out image of one of this optimizer's
        weights (backward-data transpose, sub-pixel phase merge).  Host state only: a step in flight keeps the table it was
        launched with alive (refresh_prepared's record_stream), so nothing waits here -- a settle from inside the first
        discriminator forward of a gen_update would also release the other branch stream from its wait."""
        self._prep_items.append(item)
        self._prep_table = None

    def refresh_prepared(self):
        """Rebuild every registered image from the current weights: one kernel launch on the current stream.
        The reference re-derives nothing here (cuDNN transposes inside its kernels); this build re-laid each
        weight 4-6 times per step inside the conv calls before (452 launches), now once."""
        n = len(self._prep_items)
        if n == 0 or not self.flat_p.is_cuda:
            return
        if self._prep_table is None:
            import ctypes
            from ._lib import PrepItem
            arr = (PrepItem * n)(*self._prep_items)
            host = torch.frombuffer(bytearray(ctypes.string_at(ctypes.addressof(arr), ctypes.sizeof(arr))),
                                    dtype=torch.uint8)
            self._prep_table = host.to(self.flat_p.device)
        # read on the current stream, which need not be the one it was allocated on (step_on): dropping it stays safe
        self._prep_table.record_stream(torch.cuda.current_stream(self.flat_p.device))
        ops.prepare_weights_batch(self._prep_table, n)

    def invalidate_prepared(self):
        """Call after ANY write to the weights that is not an optimizer step, a load_state_dict or an in-place op on the
        parameter / the flat buffer itself (those are seen through the tensors' version counters): `p.data.copy_(...)`,
        EMA through `.data`, a raw kernel.  Rebuilds every registered image from the current weights."""
        self.gate.settle()
        self.refresh_prepared()

    # ---- optimizer API ----------------------------------------------------------------
    def settle(self):
        """Order the current stream behind a step that step_on() left in flight; call before reading or writing flat_p /
        flat_g / flat_m / flat_v directly.  Every other way in (the methods here, the owning modules' forward, state_dict,
        load_state_dict and apply) does it itself."""
        self.gate.settle()

    def step_on(self, stream, before=None, step=None):
        """A step that runs on `stream` while the caller's stream goes on: `stream` is ordered behind the caller's, runs
        `before()` (the gradient exchange) and then `step()` (default self.step; the prepared-image refresh included), and the
        gate is armed with an event recorded behind them."""
        gate = self.gate
        gate.settle()
        ops.stream_wait(stream, torch.cuda.current_stream(stream.device))
        with torch.cuda.stream(stream):
            if before is not None:
                before()
            (step or self.step)()
            ev = torch.cuda.Event() if gate.event is None else gate.event
            ev.record(stream)
        gate.arm(ev, stream.device)

    def zero_grad(self, set_to_none=False):
        self.gate.settle()
        self.flat_g.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        self.gate.settle()
        g = self.param_groups[0]
        self._step += 1
        ops.adam_step(self.flat_p, self.flat_g, self.flat_m, self.flat_v, g["lr"], g["betas"][0], g["betas"][1],
                      g["eps"], g["weight_decay"], self._step)
        self.refresh_prepared()

    def state_dict(self):
        self.gate.settle()
        state = {}
        for i, (m, v) in enumerate(self._views):
            state[i] = {"step": torch.tensor(float(self._step)),
                        "exp_avg": m.detach().clone(memory_format=torch.contiguous_format),
                        "exp_avg_sq": v.detach().clone(memory_format=torch.contiguous_format)}
        groups = []
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != "params"}
            d["params"] = list(range(len(g["params"])))
            groups.append(d)
        return {"state": state if self._step > 0 else {}, "param_groups": groups}

    def load_state_dict(self, sd):
        self.gate.settle()
        st = sd["state"]
        with torch.no_grad():
            for i, (m, v) in enumerate(self._views):
                if i in st:
                    m.copy_(st[i]["exp_avg"])
                    v.copy_(st[i]["exp_avg_sq"])
                    self._step = int(float(st[i]["step"]))
        for g, lg in zip(self.param_groups, sd["param_groups"]):
            for k, val in lg.items():
                if k != "params":
                    g[k] = val


class FusedExtraAdam(FusedAdam):
    """ExtraAdam (scripts/extraadam.py:14-168) on the flat buffers: `extrapolation()` saves the
    parameters (first call since the last step), moves them by the Adam-style update and `step()`
    applies the update computed at the extrapolated point to the saved parameters."""

    def __init__(self, params, lr, betas, weight_decay, eps=1e-8):
        super().__init__(params, lr, betas, weight_decay, eps)
        self.flat_saved = None
        self._has_copy = False

    def bind(self, device):
        old = self.flat_saved
        super().bind(device)
        self.flat_saved = torch.zeros_like(self.flat_p)
        if old is not None and old.numel() == self.flat_saved.numel():
            self.flat_saved.copy_(old)

    def _update(self, mode):
        self.gate.settle()
        g = self.param_groups[0]
        self._step += 1
        ops.extraadam_step(self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.flat_saved, g["lr"],
                           g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self._step, mode)
        self.refresh_prepared()

    @torch.no_grad()
    def extrapolation(self):
        self._update(1 if self._has_copy else 0)
        self._has_copy = True

    @torch.no_grad()
    def step(self, closure=None):
        if not self._has_copy:
            raise RuntimeError("Need to call extrapolation before calling step.")
        self._update(2)
        self._has_copy = False


FORCE_ALLREDUCE = bool(os.environ.get("MUNIT_FORCE_ALLREDUCE"))
# Data-parallel exchange of the generator gradient in two parts (SURVEY.md section 8e "launch on a side stream to overlap
# with the remaining backward"): see GradExchange.  MUNIT_NO_OVERLAP_EXCHANGE=1 = one all-reduce after backward (A/B, tests).
OVERLAP_EXCHANGE = not os.environ.get("MUNIT_NO_OVERLAP_EXCHANGE")


def dp_size():
    """Number of data-parallel ranks (1 without a process group)."""
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def dp_world():
    """World size of the data-parallel exchange, 0 when no exchange is to be issued (no process group, or a single rank
    without MUNIT_FORCE_ALLREDUCE)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 0
    world = dist.get_world_size()
    return world if (world > 1 or FORCE_ALLREDUCE) else 0


def comm_stream(dev):
    """The communication stream of a device (one per process and device): early gradient exchanges, the deferred
    discriminator exchange + optimizer step."""
    key = (dev.type, dev.index)
    if key not in GradExchange._comm:
        GradExchange._comm[key] = torch.cuda.Stream(device=dev)
    return GradExchange._comm[key]


def all_reduce_mean(flat, world, ranges=None, works=()):
    """Mean of `flat` over the `world` ranks, in place, on the current stream: all-reduce (of `ranges` only, when stages that
    went out earlier cover the rest: `works`, waited for here), then one scale by 1 / world."""
    import torch.distributed as dist
    if ranges is None:
        dist.all_reduce(flat)
    for a, b in ranges or ():
        dist.all_reduce(flat[a:b])
    for w in works:
        w.wait()                              # on a device: the current stream waits for the communication stream
    if world > 1:
        if flat.is_cuda:
            ops.scale_(flat, 1.0 / world)
        else:
            flat.mul_(1.0 / world)


class GradExchange:
    """All-reduce (mean) of a flat gradient buffer in stages that start INSIDE the backward pass.

    Every generator weight is used by several sub-graph calls (4 encodes, 6 decodes per gen_update), so a gradient is final only
    when the LAST backward pass through its module has run.  Backward replays the forward in reverse:
      stage 1 -- the decoders' and the MLPs' last use is the pair of decodes right after the first encodes, so their gradients
        (about half of the flat buffer) are final when the gradients of the first encodes' outputs (c_a, c_b, s_a', s_b'; with
        guided == 0 also of the sampled styles, whose MLP passes have no other tensor downstream) have been formed, while the
        backward of those two encodes (about 8 % of the backward pass) is still to come;
      stage 2 -- inside that last stretch the content encoders' residual trunks (7/8 of an encoder's weights) finish first: their
        gradients are final when the gradient of the tensor ENTERING the trunk has been formed in both first encodes, while
        the down-sampling layers, the 7x7 first layers and the style encoder are still running.
    `arm(ranges, tensors)` declares a stage: it hooks the tensors, and when the last hook fires a communication stream is
    ordered behind everything enqueued so far on the producing streams (every kernel that writes the ranges has been enqueued
    by then: a node's backward-weight launch precedes the gradient it returns) and the ranges are all-reduced from it,
    asynchronously.  `finish()` (after backward, on the caller's stream) reduces what no stage covered, waits for the stages
    and scales by 1 / world.

    Every rank issues the same collectives in the same order (the autograd engine's order is a function of the graph; ranges
    of a stage in buffer order, then the rest in buffer order).  Each element is summed over the ranks exactly once either
    way; with two ranks the result is bitwise the single all-reduce's (tests), with more ranks it can differ in the last bit
    where the ring's chunk boundaries move -- as between any two bucket layouts."""

    _comm = {}

    def __init__(self, flat, world, streams=()):
        self.flat, self.world = flat, world
        self.streams = [s for s in streams if s is not None]
        self.stages, self.works = [], []

    @property
    def fired(self):
        return any(st["fired"] for st in self.stages)

    def arm(self, ranges, tensors):
        """A stage without a tensor that requires a gradient (or without elements) is dropped: finish() sends its ranges."""
        ranges = [tuple(r) for r in ranges if r[1] > r[0]]
        ts = [t for t in tensors if torch.is_tensor(t) and t.requires_grad]
        if not ranges or not ts:
            return self
        for a, b in ranges:
            for st in self.stages:
                assert all(b <= c or d <= a for c, d in st["ranges"]), "GradExchange: stages must not overlap"
        st = {"ranges": ranges, "pending": len(ts), "fired": False}
        self.stages.append(st)
        for t in ts:
            t.register_hook(lambda grad, st=st: self._hook(st))
        return self

    def _hook(self, st):
        st["pending"] -= 1
        if st["pending"] == 0:
            self._launch(st)
        return None

    def _launch(self, st):
        import torch.distributed as dist
        st["fired"] = True
        if self.flat.is_cuda:
            comm = comm_stream(self.flat.device)
            for s in self.streams:            # everything that writes the stage's ranges has been enqueued on these by now
                ops.stream_wait(comm, s)
            with torch.cuda.stream(comm):
                for a, b in st["ranges"]:
                    self.works.append(dist.all_reduce(self.flat[a:b], async_op=True))
        else:
            for a, b in st["ranges"]:
                self.works.append(dist.all_reduce(self.flat[a:b], async_op=True))

    @property
    def rest(self):
        """What no fired stage covers, in buffer order."""
        done = sorted(r for st in self.stages if st["fired"] for r in st["ranges"])
        rest, pos = [], 0
        for a, b in done:
            if a > pos:
                rest.append((pos, a))
            pos = b
        if pos < self.flat.numel():
            rest.append((pos, self.flat.numel()))
        return rest

    def finish(self):
        """Call on the stream that holds the complete gradient (after backward and the joins of the producing streams)."""
        # a stage whose hooks never fired (no tensor required grad) goes now, with what no stage covers
        all_reduce_mean(self.flat, self.world, self.rest, self.works)

BRANCH_STREAMS = not os.environ.get("MUNIT_NO_BRANCH_STREAMS")   # bench.py clears it while it times single kernels


class _Branches:
    """The a / b halves of an update on two streams.  Every stage of gen_update / dis_update consists of two
    independent halves (encode x_a | encode x_b, decode ... ), so running them on two streams lets the head and
    tail of one kernel overlap the body of another and fills the small grids of the discriminators.  Autograd
    replays each node on the stream it was recorded on, so the backward pass forks the same way.
    `share` is the cross-over point: both streams wait for each other and the tensors named become usable (and
    allocator-safe) on both.  MUNIT_NO_BRANCH_STREAMS=1 keeps everything on the caller's stream."""
    _streams = {}

    def __init__(self, dev):
        self.enabled = torch.cuda.is_available() and BRANCH_STREAMS
        if not self.enabled:
            return
        self.main = torch.cuda.current_stream(dev)
        key = (dev.type, dev.index)
        if key not in _Branches._streams:
            _Branches._streams[key] = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
        self.s = _Branches._streams[key]
        for st in self.s:
            ops.stream_wait(st, self.main)

    def run(self, k, fn):
        if not self.enabled:
            return fn()
        with torch.cuda.stream(self.s[k]):
            return fn()

    def adopt(self, *tensors):
        """Tensors that already exist on the caller's stream become usable on both branches: the fork in __init__ ordered
        the branches behind the caller's stream, so only the allocator has to be told."""
        if not self.enabled:
            return
        for t in tensors:
            if torch.is_tensor(t):
                t.record_stream(self.s[0])
                t.record_stream(self.s[1])

    def share(self, *tensors):
        if not self.enabled:
            return
        # cross-over = join into the caller's stream + fork again (the caller's stream is idle meanwhile)
        for st in self.s:
            ops.stream_wait(self.main, st)
        for st in self.s:
            ops.stream_wait(st, self.main)
        for t in tensors:
            if torch.is_tensor(t):
                t.record_stream(self.s[0])
                t.record_stream(self.s[1])

    def join(self, *tensors):
        if not self.enabled:
            return
        for st in self.s:
            ops.stream_wait(self.main, st)
        for t in tensors:
            if torch.is_tensor(t):
                t.record_stream(self.main)


BF16S_MAX_PIXELS = 1 << 23


def bf16s_refusal(hyperparameters):
    """Why `precision: bf16s` cannot run this configuration, or None.  Refused here, up front, rather than by a kernel
    entry point in the middle of a backward pass."""
    dim = hyperparameters["gen"]["dim"]
    if dim % 64 != 0:
        return ("munit_amd: precision 'bf16s' keeps the generator's activations as bf16 tensors, whose kernels "
                "work on 64-channel rows: gen.dim must be a multiple of 64 (got %d)" % dim)
    dims = (hyperparameters["input_dim_a"], hyperparameters["input_dim_b"])
    if dims != (3, 3):
        return ("munit_amd: precision 'bf16s' needs 3-channel images (input_dim_a = input_dim_b = 3, got %d and %d): the "
                "backward-weight kernels pair an fp32 image with bf16 activations for three channels only" % dims)
    # the backward-weight kernels read bf16 tensors through the 24-bit pixel arithmetic of their fast loader only
    # (conv_wgrad.hip, wgrad_form): the layers at the crop's own resolution hold batch x height x width pixels
    pixels = (int(hyperparameters.get("batch_size", 1)) * int(hyperparameters["crop_image_height"])
              * int(hyperparameters["crop_image_width"]))
    if pixels >= BF16S_MAX_PIXELS:
        return ("munit_amd: precision 'bf16s' needs batch_size x crop_image_height x crop_image_width < 2^23 = %d pixels "
                "(got %d): the bf16 backward-weight kernels address pixels with 24-bit multiplies" % (BF16S_MAX_PIXELS, pixels))
    return None


class MUNIT_Trainer(_ApplyRefreshesImages, nn.Module):
    def __init__(self, hyperparameters):
        super(MUNIT_Trainer, self).__init__()
        hyperparameters = normalize_config(hyperparameters)
        lr = hyperparameters["lr"]
        self.gen_state = hyperparameters["gen_state"]
        self.guided = hyperparameters["guided"]
        self.newsize = hyperparameters["crop_image_height"]
        self.semantic_w = hyperparameters["semantic_w"] > 0
        self.recon_mask = hyperparameters["recon_mask"] == 1
        self.dann_scheduler = None
        self.full_adaptation = hyperparameters["adaptation"]["full_adaptation"] == 1
        self.hyperparameters = hyperparameters
        self.iterations = 0
        # build extension (no reference counterpart): `precision: bf16` = BASELINE.json config #3 -- the conv /
        # linear contractions multiply bf16-rounded operands with fp32 accumulation; tensors, norm statistics,
        # losses and the optimizer stay fp32.  Default: the reference's fp32 arithmetic.
        # `precision: bf16s` = bf16 STORAGE on top of that: the content encoders write bf16 activations, and the content
        # code carries the type through the decoders up to the fp32 image head; norm statistics, AdaIN parameters,
        # weights, gradients of weights, optimizer state, losses, the style encoder and the discriminators stay fp32.
        self.precision = hyperparameters.get("precision", "f32")
        ops.set_compute(self.precision)
        # build extension, opt-in (`reuse_dis_forward: 1`): dis_update and the gen_update that follows it in the same
        # iteration (scripts/train.py:182-187) run the SAME generator forward -- encode x_a, encode x_b, decode x_ba,
        # decode x_ab -- on the same images with the same generator weights (only the discriminators step in between);
        # the reference computes it twice (trainer.py:1146-1179 under no autograd, then trainer.py:366-390).  With this
        # switch dis_update keeps that forward and its autograd tape and gen_update continues from it when it is handed
        # the very same tensors: 11 % fewer multiply-accumulates per step; the forward values (and therefore every
        # loss) are the same numbers, the gradients agree to fp32 summation order (the kept nodes are older on the autograd
        # tape, so the uses of a shared weight accumulate in another order).  Off by default: the benchmark's step is
        # defined on the reference's sequence of computations.
        self.reuse_dis_forward = bool(hyperparameters.get("reuse_dis_forward", 0))
        self._fwd_cache = None
        self.fwd_reused = False     # whether the last gen_update continued from dis_update's forward
        self.last_exchange = None   # the GradExchange of the last data-parallel gen_update (introspection)

        optimizer = FusedExtraAdam if "extra" in hyperparameters["optimizer"] else FusedAdam  # trainer.py:41-45

        def make_opt(*modules):
            """the optimizer over the trainable parameters of `modules`, in their order"""
            opt = optimizer([p for m in modules for p in m.parameters() if p.requires_grad], lr=lr,
                            betas=(hyperparameters["beta1"], hyperparameters["beta2"]),
                            weight_decay=hyperparameters["weight_decay"])
            for m in modules:
                if isinstance(m, MsImageDis):   # their forward and (load_)state_dict wait for a step of opt still in flight
                    m.follow(opt.gate)
            return opt
        self.domain_classif_ab = hyperparameters.get("domain_adv_w", 0) > 0
        self.use_classifier_sr = hyperparameters["adaptation"]["dfeat_lambda"] > 0
        self.train_seg = hyperparameters["adaptation"]["sem_seg_lambda"] > 0
        self.use_output_classifier_sr = hyperparameters["adaptation"]["output_classifier_lambda"] > 0
        self._check_aux(hyperparameters)
        self._check_featda(hyperparameters, self.use_classifier_sr)
        self._check_outda(hyperparameters, self.use_output_classifier_sr)
        self._check_seghead(hyperparameters, self.train_seg)
        self._check_sn(hyperparameters)
        self.use_vgg = hyperparameters.get("vgg_w", 0) > 0
        if self.use_vgg:
            self._check_vgg(hyperparameters)

        if self.gen_state == 0:
            self.gen_a = AdaINGen(hyperparameters["input_dim_a"], hyperparameters["gen"])
            self.gen_b = AdaINGen(hyperparameters["input_dim_b"], hyperparameters["gen"])
        elif self.gen_state == 1:
            self.gen = AdaINGen_double(hyperparameters["input_dim_a"], hyperparameters["gen"])
        else:
            raise ValueError("self.gen_state unknown value: %r" % (self.gen_state,))
        if self.precision == "bf16s":
            why = bf16s_refusal(hyperparameters)
            if why is not None:
                raise ValueError(why)
            for m in self.modules():
                if isinstance(m, ContentEncoder):
                    m.store_dtype = torch.bfloat16
        self.dis_a = MsImageDis(hyperparameters["input_dim_a"], hyperparameters["dis"])
        self.dis_b = MsImageDis(hyperparameters["input_dim_b"], hyperparameters["dis"])
        self.instancenorm = InstanceNorm2d(512)
        self.style_dim = hyperparameters["gen"]["style_dim"]

        # fixed display noise (trainer.py:93-95); kept on the host until a device is known
        display_size = int(hyperparameters["display_size"])
        self.s_a = torch.randn(display_size, self.style_dim, 1, 1)
        self.s_b = torch.randn(display_size, self.style_dim, 1, 1)

        self.dis_opt = make_opt(self.dis_a, self.dis_b)
        self.gen_opt = make_opt(self.gen_a, self.gen_b) if self.gen_state == 0 else make_opt(self.gen)
        self.dis_scheduler = get_scheduler(self.dis_opt, hyperparameters)
        self.gen_scheduler = get_scheduler(self.gen_opt, hyperparameters)

        # Network weight initialization (trainer.py:124-127)
        self.apply(weights_init(hyperparameters["init"]))
        self.dis_a.apply(weights_init("gaussian"))
        self.dis_b.apply(weights_init("gaussian"))

        # semantic-consistency loss (trainer.py:136-142): the user's Resnet34_8s checkpoint, frozen, in eval mode
        self.segmentation_model = None
        if self.semantic_w:
            self._check_semantic(hyperparameters)
            self.segmentation_model = load_segmentation_model(hyperparameters["semantic_ckpt_path"], 19)

        # domain-invariant perceptual loss (trainer.py:129-134): the VGG16 of <vgg_model_path>/models/vgg16.weight, frozen, in
        # eval mode.  A plain attribute, not a sub-module: state_dict() is the same with and without the loss, and the
        # network makes its own device copy of the weights at first use (Vgg16.weights), so .to() need not move it.
        self.__dict__["vgg"] = load_vgg16(hyperparameters["vgg_model_path"] + "/models") if self.use_vgg else None

        # feature classifiers of the simulated / real adaptation (trainer.py:161-179): one optimizer over both, a scheduler
        # that update_learning_rate never steps, nothing of them in save / resume
        if self.use_classifier_sr:
            self.domain_classifier_sr_b = domainClassifier(256)
            self.domain_classifier_sr_a = domainClassifier(256)
            self.classif_opt_sr = make_opt(self.domain_classifier_sr_a, self.domain_classifier_sr_b)
            self.domain_classifier_sr_a.apply(weights_init("gaussian"))
            self.domain_classifier_sr_b.apply(weights_init("gaussian"))
            self.classif_sr_scheduler = get_scheduler(self.classif_opt_sr, hyperparameters)

        # output classifiers of the simulated / real adaptation (trainer.py:181-201): both on input_dim_a, one optimizer over
        # both, a scheduler that update_learning_rate never steps, nothing of them in save / resume
        if self.use_output_classifier_sr:
            self.output_classifier_sr_a = MsImageDis(hyperparameters["input_dim_a"], hyperparameters["dis"])
            self.output_classifier_sr_b = MsImageDis(hyperparameters["input_dim_a"], hyperparameters["dis"])
            self.output_classif_opt_sr = make_opt(self.output_classifier_sr_a, self.output_classifier_sr_b)
            self.output_classifier_sr_a.apply(weights_init("gaussian"))
            self.output_classifier_sr_b.apply(weights_init("gaussian"))
            self.output_scheduler_sr = get_scheduler(self.output_classif_opt_sr, hyperparameters)

        # segmentation head on the content codes (trainer.py:203-223): created after the initialisation above, so it keeps the
        # checkpoint's weights; its own optimizer, a scheduler that update_learning_rate never steps, nothing in save / resume
        if self.train_seg:
            self.segmentation_head = load_segmentation_head(hyperparameters["semantic_ckpt_path"])
            self.segmentation_opt = make_opt(self.segmentation_head)
            self.scheduler_seg = get_scheduler(self.segmentation_opt, hyperparameters)

        self._consts = {}
        self._bind(torch.device("cpu"))

    # ------------------------------------------------------------------------------------
    @staticmethod
    def _check_aux(hp, construct=True):
        """construct False (gen_update): the both-weights rule of the output classifiers is a rule of construction -- a
        trainer that owns them may be handed output_adv_lambda 0 for a step."""
        bad = []
        if hp.get("vgg_w", 0) > 0 and not hp.get("vgg_model_path"):
            bad.append("vgg_w (without a vgg_model_path that holds models/vgg16.weight)")
        if hp.get("semantic_w", 0) > 0 and not hp.get("semantic_ckpt_path"):
            bad.append("semantic_w (without a semantic_ckpt_path)")
        if hp.get("domain_adv_w", 0) > 0:
            bad.append("domain_adv_w")
        if hp["adaptation"].get("sem_seg_lambda", 0) > 0 and not hp.get("semantic_ckpt_path"):
            bad.append("adaptation.sem_seg_lambda (without a semantic_ckpt_path: the head starts from that checkpoint's layer4)")
        ocl = hp["adaptation"].get("output_classifier_lambda", 0) > 0
        oadv = hp["adaptation"].get("output_adv_lambda", 0) > 0
        if construct and oadv and not ocl:
            bad.append("adaptation.output_adv_lambda (without adaptation.output_classifier_lambda there are no classifiers "
                       "to fool: set both)")
        if construct and ocl and not oadv:
            bad.append("adaptation.output_classifier_lambda (without adaptation.output_adv_lambda it trains classifiers that "
                       "nothing reads: set both)")
        if bad:
            raise NotImplementedError(
                "munit_amd: set these weights to 0: " + ", ".join(bad) + ".  domain_adv_w cannot run in the reference "
                "either (the a/b domain classifier's loss builds a 4-element target for any batch size), and the reference's "
                "load_vgg16 raises unconditionally: vgg_w needs the file it would have cached, "
                "<vgg_model_path>/models/vgg16.weight; semantic_w and adaptation.sem_seg_lambda need the user's Resnet34_8s "
                "checkpoint (semantic_ckpt_path)")

    @staticmethod
    def _check_vgg(hp, built=True):
        """Refusals of vgg_w > 0, before any device work.  built: whether this trainer was constructed with the weight and
        a vgg_model_path (it then owns the network)."""
        if not built:
            raise ValueError("munit_amd: vgg_w > 0 needs a trainer constructed with vgg_w > 0 and a vgg_model_path (the VGG16 "
                             "is loaded under that weight)")
        if hp.get("precision", "f32") != "f32":
            raise NotImplementedError("munit_amd: vgg_w > 0 runs in fp32 only (precision %r)" % hp["precision"])
        check_vgg_hw(hp["crop_image_height"], hp["crop_image_width"])

    @staticmethod
    def _check_featda(hp, built):
        """Refusals of adaptation.adv_lambda / adaptation.dfeat_lambda, before any device work.  built: whether this trainer
        was constructed with dfeat_lambda > 0 (it then owns the classifiers)."""
        ad = hp["adaptation"]
        adv, dfeat = ad.get("adv_lambda", 0) > 0, ad.get("dfeat_lambda", 0) > 0
        if adv and not (dfeat and built):
            raise ValueError("munit_amd: adaptation.adv_lambda > 0 needs adaptation.dfeat_lambda > 0 at construction (the "
                             "classifiers the generator is to fool are built and trained under dfeat_lambda)")
        if not (adv or dfeat):
            return
        if hp.get("precision", "f32") != "f32":
            raise NotImplementedError("munit_amd: adaptation.adv_lambda / adaptation.dfeat_lambda run in fp32 only "
                                      "(precision %r)" % hp["precision"])
        if dp_size() > 1 and not ad.get("data_parallel", 0):
            raise NotImplementedError("munit_amd: adaptation.adv_lambda / adaptation.dfeat_lambda are not implemented for "
                                      "data-parallel training (world size %d): the classifiers' gradients and batch "
                                      "statistics are not exchanged; set adaptation.data_parallel: 1 to exchange them (the "
                                      "classifiers' batch norms then take their statistics over all ranks)" % dp_size())
        n = hp["gen"]["n_downsample"]
        try:
            domainClassifier.check_code_hw(hp["crop_image_height"] >> n, hp["crop_image_width"] >> n)
        except ValueError as e:
            raise ValueError("munit_amd: adaptation.dfeat_lambda / adaptation.adv_lambda cannot run at crop %dx%d with "
                             "gen.n_downsample %d: %s" % (hp["crop_image_height"], hp["crop_image_width"], n, e)) from None

    @staticmethod
    def _check_outda(hp, built, update=False):
        """Refusals of adaptation.output_adv_lambda / adaptation.output_classifier_lambda, before any device work.  built:
        whether this trainer was constructed with both weights (it then owns the classifiers); update: the check of
        output_domain_classifier_sr_update, which runs whatever the weights of `hp` are."""
        adv = hp["adaptation"].get("output_adv_lambda", 0) > 0
        if adv and hp.get("dis", {}).get("gan_type") == "nsgan":
            raise NotImplementedError("munit_amd: dis.gan_type: nsgan cannot run together with adaptation.output_adv_lambda > 0: "
                                      "the fooling term is MsImageDis.calc_gen_loss_sr, whose nsgan branch names an undefined "
                                      "variable in the reference (NameError): there is no behaviour to reproduce")
        if (adv or update) and not built:
            raise ValueError("munit_amd: adaptation.output_adv_lambda > 0 needs a trainer constructed with "
                             "adaptation.output_classifier_lambda > 0 and adaptation.output_adv_lambda > 0 (the classifiers "
                             "the generator is to fool are built and trained under those)")
        if not (adv or update or built):
            return
        keys = "adaptation.output_adv_lambda / adaptation.output_classifier_lambda"
        if hp.get("precision", "f32") != "f32":
            raise NotImplementedError("munit_amd: %s run in fp32 only (precision %r)" % (keys, hp["precision"]))
        if dp_size() > 1 and not hp["adaptation"].get("data_parallel", 0):
            raise NotImplementedError("munit_amd: %s are not implemented for data-parallel training (world size %d): the "
                                      "classifiers' gradients are not exchanged; set adaptation.data_parallel: 1 to exchange "
                                      "them" % (keys, dp_size()))
        if "extra" in hp.get("optimizer", "adam"):
            raise NotImplementedError("munit_amd: %s are not implemented for optimizer %r: the reference's update calls "
                                      "step() without extrapolation(), on which its ExtraAdam raises"
                                      % (keys, hp["optimizer"]))

    @staticmethod
    def _check_sn(hp):
        """Refusals of dis.norm: sn (spectral normalisation of the discriminators and output classifiers), before anything is
        built."""
        if hp.get("dis", {}).get("norm") != "sn":
            return
        if hp.get("precision", "f32") != "f32":
            raise NotImplementedError("munit_amd: dis.norm: sn runs in fp32 only (precision %r)" % hp["precision"])
        if dp_size() > 1:
            raise NotImplementedError("munit_amd: dis.norm: sn is not implemented for data-parallel training (world size %d): "
                                      "every rank would draw and iterate its own weight_u / weight_v, and how they are to be "
                                      "exchanged is not settled" % dp_size())

    @staticmethod
    def _check_seghead(hp, built, update=False):
        """Refusals of adaptation.sem_seg_lambda, before any device work.  built: whether this trainer was constructed with
        the weight (it then owns the head); update: the check of segmentation_head_update."""
        if update and not built:
            raise ValueError("munit_amd: segmentation_head_update needs a trainer constructed with "
                             "adaptation.sem_seg_lambda > 0 (and a semantic_ckpt_path): the head is built under that weight")
        if not built:
            return
        key = "adaptation.sem_seg_lambda"
        if hp.get("precision", "f32") != "f32":
            raise NotImplementedError("munit_amd: %s runs in fp32 only (precision %r)" % (key, hp["precision"]))
        if "extra" in hp.get("optimizer", "adam"):
            raise NotImplementedError("munit_amd: %s is not implemented for optimizer %r: the reference's update calls "
                                      "step() without extrapolation(), on which its ExtraAdam raises" % (key, hp["optimizer"]))
        if dp_size() > 1:
            raise NotImplementedError("munit_amd: %s is not implemented for data-parallel training (world size %d), also "
                                      "under adaptation.data_parallel: 1: the head's gradients are not exchanged and its batch "
                                      "norms take their statistics from one rank's batch; spanning them over the ranks is a "
                                      "later change" % (key, dp_size()))
        h, w, n = hp["crop_image_height"], hp["crop_image_width"], hp["gen"]["n_downsample"]
        if h != w:
            raise ValueError("munit_amd: %s needs a square crop (the reference up-samples the head's output to "
                             "(crop_image_height, crop_image_height)); got %dx%d" % (key, h, w))
        if 2 ** n not in (1, 2, 4, 8):
            raise ValueError("munit_amd: %s needs gen.n_downsample in 0..3 (the head kernel up-samples by 1, 2, 4 or 8); "
                             "got %d" % (key, n))
        if h % 2 ** n or (h >> n) % 4 or (w >> n) % 4:
            raise ValueError("munit_amd: %s needs a content code whose extents are multiples of 4 (layer4's dilation-4 "
                             "convolutions run on its 4 x 4 phases): crop %dx%d with gen.n_downsample %d gives %gx%g"
                             % (key, h, w, n, h / 2 ** n, w / 2 ** n))

    @staticmethod
    def _check_semantic(hp):
        if hp.get("precision", "f32") != "f32":
            raise NotImplementedError("munit_amd: semantic_w > 0 runs in fp32 only (precision %r)" % hp["precision"])
        h, w = hp["crop_image_height"], hp["crop_image_width"]
        if h != w:
            raise ValueError("munit_amd: semantic_w > 0 needs a square crop (the reference resizes the mask to "
                             "(crop_image_height, crop_image_height)); got %dx%d" % (h, w))
        if h % 32:
            raise ValueError("munit_amd: semantic_w > 0 needs a crop that is a multiple of 32 (the segmentation network's "
                             "1/8-resolution features split into 4 x 4 phases); got %d" % h)

    @staticmethod
    def _check_semantic_gt(x_a, gt_a, gt_b, names=("semantic_gt_a", "semantic_gt_b")):
        """Argument checks of semantic_gt_a / semantic_gt_b (no device work): None when neither is given, else the two maps
        viewed as (B, H, W).  names: what the caller calls the two maps (segmentation_head_update: target_a / target_b)."""
        if gt_a is None and gt_b is None:
            return None
        if gt_a is None or gt_b is None:
            raise ValueError("munit_amd: %s and %s must be given together (got only %s)"
                             % (names[0], names[1], names[1] if gt_a is None else names[0]))
        b, _, h, w = x_a.shape
        out = []
        for name, g in zip(names, (gt_a, gt_b)):
            if not torch.is_tensor(g) or g.is_complex() or g.dtype == torch.bool:
                raise ValueError("munit_amd: %s must be a tensor of a real dtype, got %s"
                                 % (name, g.dtype if torch.is_tensor(g) else type(g)))
            if tuple(g.shape) not in ((b, 1, h, w), (b, h, w)):
                raise ValueError("munit_amd: %s must be (B, 1, H, W) or (B, H, W) at the image size %s, got %s"
                                 % (name, (b, h, w), tuple(g.shape)))
            g = g.detach().reshape(b, h, w)
            if g.device.type == "cpu":      # the reference passes host tensors: those are range-checked here
                bad = bool((~torch.isfinite(g)).any()) if g.is_floating_point() else False
                if not bad:
                    t = g.long()            # .type(torch.long), trainer.py:734
                    bad = int(t.min()) < 0 or int(t.max()) > 9
                if bad:
                    raise ValueError("munit_amd: %s holds labels outside 0..9 (the simulator's 10 classes)" % name)
            out.append(g)
        return out

    @staticmethod
    def _gt_to_device(gts, dev):
        """float32 (2B, H, W) on the device, each value already truncated as .type(torch.long) would."""
        conv = []
        for g in gts:
            if g.is_floating_point() and g.dtype != torch.float32:
                g = g.trunc()               # a float64 9.9999999999 must not round up to 10 in float32
            conv.append(g.to(dev, torch.float32))
        return torch.cat(conv).contiguous()

    def _semantic_loss(self, x_a, x_b, x_ab, x_ba, mask_a, mask_b, gt=None):
        """seg(x_a, x_ab, mask_a) + seg(x_b, x_ba, mask_b) (trainer.py:504-509) as one pass over each image pair.
        gt: the ground-truth maps of both pairs (2B, H, W) float32, or None for pseudo-labels."""
        mask = None
        if not self.full_adaptation and (mask_a is not None or mask_b is not None):
            if mask_a is None or mask_b is None:
                raise ValueError("munit_amd: the masked semantic loss needs both mask_a and mask_b")
            for m in (mask_a, mask_b):
                if m.dim() != 4 or m.shape[1] != 1 or m.shape[2:] != x_a.shape[2:]:
                    raise ValueError("munit_amd: semantic-loss masks must be (B, 1, H, W) at the image size %s, got %s"
                                     % (tuple(x_a.shape[2:]), tuple(m.shape)))
            mask = torch.cat([mask_a.float(), mask_b.float()]).contiguous()
        loss, _ = seg_loss(self.segmentation_model, [x_a, x_b], [x_ab, x_ba], mask, gt)
        return loss

    def _bind(self, device):
        self.dis_opt.bind(device)
        self.gen_opt.bind(device)
        if self.use_classifier_sr:
            self.classif_opt_sr.bind(device)
        if self.use_output_classifier_sr:
            self.output_classif_opt_sr.bind(device)
        if self.train_seg:
            self.segmentation_opt.bind(device)
        self._consts = {}
        # flat-gradient ranges of the decoders and MLPs (final before the first encodes' backward: GradExchange)
        gens = [self.gen] if self.gen_state == 1 else [self.gen_a, self.gen_b]
        early = {id(p) for g in gens for n, p in g.named_parameters() if n.startswith("dec") or n.startswith("mlp")}
        self._early_ranges = self.gen_opt.ranges_of(lambda p: id(p) in early)
        # ... and of the content encoders' residual trunks (final before the first encodes' down-sampling layers run backward)
        trunk = {id(p) for k in (1, 2) for p in self._content_enc(k).model[-1].parameters()}
        self._trunk_ranges = self.gen_opt.ranges_of(lambda p: id(p) in trunk)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        p = next(self.dis_a.parameters())
        self._bind(p.device)
        self.s_a = self.s_a.to(p.device)
        self.s_b = self.s_b.to(p.device)
        return out

    def _const(self, value, device):
        key = (float(value), device)
        t = self._consts.get(key)
        if t is None:
            t = torch.full((), float(value), dtype=torch.float32, device=device)
            self._consts[key] = t
        return t

    # ---- optimizer steps (trainer.py:252-268) -----------------------------------------
    def _opt_step(self, opt):
        if "extra" in self.hyperparameters["optimizer"] and (self.iterations % 2 == 0):
            opt.extrapolation()
        else:
            opt.step()

    def dis_opt_step(self):
        """ExtraAdam extrapolates on even iterations and steps on odd ones (trainer.py:252-259)."""
        self._opt_step(self.dis_opt)

    def gen_opt_step(self):
        self._opt_step(self.gen_opt)

    def classif_opt_sr_step(self):
        """trainer.py:243-250."""
        self._opt_step(self.classif_opt_sr)

    def output_classif_opt_sr_step(self):
        """trainer.py:234-241.  Exists as in the reference, whose update does not call it either."""
        self._opt_step(self.output_classif_opt_sr)

    def segmentation_opt_step(self):
        """trainer.py:270-277.  Exists as in the reference, whose update does not call it either."""
        self._opt_step(self.segmentation_opt)

    # ---- criteria (trainer.py:279-305) ------------------------------------------------
    def recon_criterion(self, input, target):
        return ops.l1_mean(input, target)

    def recon_criterion_mask(self, input, target, mask):
        return ops.l1_mean(input, target, mask)

    # ---- simulated / real feature classifiers (trainer.py:638-667, 1237-1265) -----------
    @staticmethod
    def _sr_target(domain_synth, fool):
        return 0.5 if fool else (0.0 if domain_synth else 1.0)

    @staticmethod
    def _bn_world(hp):
        """World size over which the feature classifiers' batch norms take their statistics (ops.bn_world): the process
        group's under adaptation.data_parallel: 1 with more than one rank, else 0 (the process's own batch).  The ranks start
        from identical classifiers the way they start from identical generators: every rank constructs its trainer under
        the same seed (bench.py, tests/test_gpu_dp.py); the batch-norm buffers start at 0 / 1 and move by the joined
        statistics, which are bitwise the same on every rank."""
        return dp_size() if (hp["adaptation"].get("data_parallel", 0) and dp_size() > 1) else 0

    def compute_classifier_sr_loss(self, c_a, c_b, domain_synth=False, fool=False, need_weight_grads=True):
        """mean((cls_a(c_a) - t)^2) + mean((cls_b(c_b) - t)^2), t = 0.5 to fool, else 0 for synthetic and 1 for real codes.
        need_weight_grads False (build extension): the backward pass forms the gradients of c_a / c_b only."""
        if not self.use_classifier_sr:
            raise ValueError("munit_amd: compute_classifier_sr_loss needs a trainer built with adaptation.dfeat_lambda > 0")
        t = self._sr_target(domain_synth, fool)
        with ops.bn_world(self._bn_world(self.hyperparameters)):
            output_a = self.domain_classifier_sr_a(c_a, need_weight_grads)
            output_b = self.domain_classifier_sr_b(c_b, need_weight_grads)
        return ops.scalar_sum([ops.mse_const(output_a, t), ops.mse_const(output_b, t)])

    def domain_classifier_sr_update(self, x_a, x_b, domain_synth, lambda_classifier, step, comet_exp=None):
        """trainer.py:1237-1265.  The codes are detached there: the encodes run without a tape, and only the content
        encoders run (the style codes the reference also forms are never used)."""
        ops.set_compute(self.precision)
        if not self.use_classifier_sr:
            raise ValueError("munit_amd: domain_classifier_sr_update needs a trainer built with adaptation.dfeat_lambda > 0")
        self._check_featda(self.hyperparameters, True)
        self.classif_opt_sr.zero_grad()
        dev = x_a.device
        x_a, x_b = ops.nhwc(x_a), ops.nhwc(x_b)
        t = self._sr_target(domain_synth, False)
        br = _Branches(dev)
        br.adopt(x_a, x_b)

        def half(x, k, cls):
            with torch.no_grad():
                c = self._content_enc(k)(x)
            return ops.mse_const(cls(c.detach()), t)

        # data parallel: the batch norms exchange their statistics inside both passes -- a before b in the forward (the host
        # issues the two halves one after the other), the engine's order in the backward: the same sequence on every rank
        with ops.bn_world(self._bn_world(self.hyperparameters)):
            l_a = br.run(0, lambda: half(x_a, 1, self.domain_classifier_sr_a))
            l_b = br.run(1, lambda: half(x_b, 2, self.domain_classifier_sr_b))
        br.join(l_a, l_b)
        loss = ops.scalar_sum([l_a, l_b])
        self.loss_classifier_sr_update = loss.detach()      # unweighted; the reference logs lambda_classifier * loss
        torch.autograd.backward([loss], [self._const(lambda_classifier, dev)])
        br.join()
        ops.join_side_streams()
        self._all_reduce_mean(self.classif_opt_sr.flat_g)   # in line on the caller's stream: 4.8 MB, nothing to overlap with
        self.classif_opt_sr_step()
        if comet_exp is not None and self.iterations % 100 == 0:
            comet_exp.log_metric("loss_classifier_sr", (lambda_classifier * self.loss_classifier_sr_update).cpu(), step=step)

    # ---- simulated / real output classifiers (trainer.py:1267-1284) ----------------------
    def output_domain_classifier_sr_update(self, x_ar, x_as, x_br, x_bs, hyperparameters, step, comet_exp=None):
        """trainer.py:1267-1284: cls_b.calc_dis_loss_sr(x_bs, x_br) + cls_a.calc_dis_loss_sr(x_as, x_ar), times
        output_classifier_lambda, then the optimizer's plain step() (never extrapolation(), as in the reference).
        update_learning_rate, save and resume are unchanged by these classifiers, as in the reference."""
        ops.set_compute(self.precision)
        self._check_outda(self.hyperparameters, self.use_output_classifier_sr, update=True)
        lam = hyperparameters["adaptation"]["output_classifier_lambda"]
        self.output_classif_opt_sr.zero_grad()
        dev = x_ar.device
        x_ar, x_as, x_br, x_bs = ops.nhwc(x_ar), ops.nhwc(x_as), ops.nhwc(x_br), ops.nhwc(x_bs)
        br = _Branches(dev)
        br.adopt(x_ar, x_as, x_br, x_bs)
        l_a = br.run(0, lambda: self.output_classifier_sr_a.calc_dis_loss_sr(x_as, x_ar))
        l_b = br.run(1, lambda: self.output_classifier_sr_b.calc_dis_loss_sr(x_bs, x_br))
        br.join(l_a, l_b)
        loss = ops.scalar_sum([l_b, l_a])
        self.loss_output_classifier_sr_update = loss.detach()      # unweighted; the reference logs lambda * loss
        torch.autograd.backward([loss], [self._const(lam, dev)])
        br.join()
        ops.join_side_streams()
        self._all_reduce_mean(self.output_classif_opt_sr.flat_g)      # in line on the caller's stream
        self.output_classif_opt_sr.step()
        if comet_exp is not None and self.iterations % 100 == 0:
            comet_exp.log_metric("loss_output_classifier_sr", (lam * self.loss_output_classifier_sr_update).cpu(), step=step)

    # ---- segmentation head on the content codes (trainer.py:1286-1324) --------------------
    def segmentation_head_update(self, x_a, x_b, target_a, target_b, lamb, comet_exp=None):
        """trainer.py:1286-1324: (CE(up(head(c_a)), target_a) + CE(up(head(c_b)), target_b)) * lamb, then the optimizer's plain
        step() (never extrapolation()).  Only the content encoders run, without a tape: the gradient the reference sends into
        the encoders is zeroed by the next gen_update before anything reads it.  targets: (B, 1, H, W) or (B, H, W) label maps
        of the simulator's 10 classes at the crop size, on the images' device."""
        ops.set_compute(self.precision)
        self._check_seghead(self.hyperparameters, self.train_seg, update=True)
        dev = x_a.device
        b, _, h, w = x_a.shape
        if (h, w) != (self.newsize, self.newsize) or x_b.shape != x_a.shape:
            raise ValueError("munit_amd: segmentation_head_update needs both images at the crop size %dx%d (the head's output "
                             "is up-sampled to it), got %s and %s" % (self.newsize, self.newsize, tuple(x_a.shape), tuple(x_b.shape)))
        if target_a is None or target_b is None:
            raise ValueError("munit_amd: segmentation_head_update needs both label maps (target_a and target_b)")
        gts = self._check_semantic_gt(x_a, target_a, target_b, ("target_a", "target_b"))
        for name, g in zip(("target_a", "target_b"), gts):
            if g.device != dev:
                raise ValueError("munit_amd: %s must live on the images' device %s, got %s" % (name, dev, g.device))
        gt = self._gt_to_device(gts, dev)
        scale = 2 ** self.hyperparameters["gen"]["n_downsample"]
        self.segmentation_opt.zero_grad()
        x_a, x_b = ops.nhwc(x_a), ops.nhwc(x_b)
        with torch.no_grad():
            c_a = self._content_enc(1)(x_a)
            c_b = self._content_enc(2)(x_b)
        loss = seg_head_loss(self.segmentation_head, c_a.detach(), c_b.detach(), gt[:b], gt[b:], scale)
        self.loss_semantic_head = ops.weighted_sum([loss.detach()], [lamb])      # the weighted loss, as the reference logs it
        torch.autograd.backward([loss], [self._const(lamb, dev)])
        ops.join_side_streams()
        self.segmentation_opt.step()
        self._log(comet_exp, ["loss_semantic_head"])

    # ---- generator dispatch -----------------------------------------------------------
    def _enc(self, x, k):
        if self.gen_state == 1:
            return self.gen.encode(x, k)
        return (self.gen_a if k == 1 else self.gen_b).encode(x)

    def _content_enc(self, k):
        if self.gen_state == 1:
            return self.gen.enc1_content if k == 1 else self.gen.enc2_content
        return (self.gen_a if k == 1 else self.gen_b).enc_content

    def _enc_keep(self, x, k):
        """encode, also returning the tensor that enters the content encoder's residual trunk (GradExchange stage 2)."""
        enc = self._content_enc(k)
        enc.keep_trunk_in = True
        try:
            c, s = self._enc(x, k)
            t = enc.trunk_in
        finally:
            enc.keep_trunk_in, enc.trunk_in = False, None
        return c, s, t

    def _dec(self, c, s, k):
        if self.gen_state == 1:
            return self.gen.decode(c, s, k)
        return (self.gen_a if k == 1 else self.gen_b).decode(c, s)

    def forward(self, x_a, x_b):
        """trainer.py:307-334."""
        ops.set_compute(self.precision)
        self.eval()
        with torch.no_grad():
            s_a, s_b = self.s_a.to(x_a.device), self.s_b.to(x_a.device)
            c_a, _ = self._enc(x_a, 1)
            c_b, _ = self._enc(x_b, 2)
            x_ba = self._dec(c_b, s_a, 1)
            x_ab = self._dec(c_a, s_b, 2)
        self.train()
        return x_ab, x_ba

    @staticmethod
    def _all_reduce_mean(flat):
        """Data-parallel exchange: one all-reduce (RCCL over xGMI) of the flat gradient.  MUNIT_FORCE_ALLREDUCE=1
        issues it at world size 1 too (a 1-GPU box then exercises the RCCL path; the result is unchanged)."""
        world = dp_world()
        if world:
            all_reduce_mean(flat, world)

    # ---- gen_update (trainer.py:336-561) -----------------------------------------------
    def gen_update(self, x_a, x_b, hyperparameters, mask_a=None, mask_b=None, comet_exp=None, synth=False,
                   semantic_gt_a=None, semantic_gt_b=None):
        ops.set_compute(self.precision)
        hp = hyperparameters
        pair_term = bool(synth) and hp.get("recon_synth_w", 0) > 0
        gts = self._check_semantic_gt(x_a, semantic_gt_a, semantic_gt_b)
        if not self.semantic_w:
            gts = None                         # ignored, as in the reference (trainer.py:505-510)
        if gts is not None and x_a.device.type != "cuda":
            raise NotImplementedError("munit_amd: semantic_gt_a / semantic_gt_b run on the device only (there is no host "
                                      "path for any loss); move the trainer and the images to a HIP device")
        vgg_on = hp.get("vgg_w", 0) > 0
        if vgg_on:     # ahead of _check_aux: a trainer built without the network is the caller's error whatever else hp lacks
            self._check_vgg(dict(hp, crop_image_height=x_a.shape[2], crop_image_width=x_a.shape[3]), self.vgg is not None)
        self._check_aux(normalize_config(hp), construct=False)
        self._check_featda(hp, self.use_classifier_sr)
        self._check_outda(hp, self.use_output_classifier_sr)
        fool_sr = hp["adaptation"]["adv_lambda"] > 0
        fool_out = hp["adaptation"]["output_adv_lambda"] > 0
        self.gen_opt.zero_grad()
        # the reference draws these even when guided == 1 leaves them unused (trainer.py:366-367)
        s_a = torch.randn(x_a.size(0), self.style_dim, 1, 1)
        s_b = torch.randn(x_b.size(0), self.style_dim, 1, 1)
        dev = x_a.device
        fwd_key = self._fwd_key(x_a, x_b)      # of the caller's tensors (the layout conversion below may copy)
        x_a, x_b = ops.nhwc(x_a), ops.nhwc(x_b)

        world = dp_world()
        overlap = bool(world and OVERLAP_EXCHANGE)      # stages of the gradient exchange start inside backward (GradExchange)
        d_params = list(self.dis_a.parameters()) + list(self.dis_b.parameters())
        if fool_out:        # ... and so would the output classifiers' (zeroed by the next update's zero_grad, trainer.py:1271)
            d_params += list(self.output_classifier_sr_a.parameters()) + list(self.output_classifier_sr_b.parameters())
        d_params = [p for p in d_params if p.requires_grad]     # dis.norm sn: weight_u / weight_v never take a gradient
        for p in d_params:  # D weight gradients made here would be discarded (trainer.py:1145)
            p.requires_grad_(False)
        try:
            br = _Branches(dev)
            br.adopt(x_a, x_b, mask_a, mask_b)
            cached, self._fwd_cache = self._fwd_cache, None
            reuse = (cached is not None and self.guided == 1 and cached[0] == fwd_key)
            self.fwd_reused = reuse
            trunk_a = trunk_b = None
            if reuse:      # the forward dis_update just ran on these tensors with these generator weights
                c_a, s_a_prime, c_b, s_b_prime, x_ba_kept, x_ab_kept = cached[1]
                br.adopt(c_a, s_a_prime, c_b, s_b_prime, x_ba_kept, x_ab_kept)
            elif overlap:  # also keep the tensors entering the residual trunks: their gradients open stage 2 of the exchange
                c_a, s_a_prime, trunk_a = br.run(0, lambda: self._enc_keep(x_a, 1))
                c_b, s_b_prime, trunk_b = br.run(1, lambda: self._enc_keep(x_b, 2))
            else:
                c_a, s_a_prime = br.run(0, lambda: self._enc(x_a, 1))
                c_b, s_b_prime = br.run(1, lambda: self._enc(x_b, 2))
            del cached
            x_a_recon = br.run(0, lambda: self._dec(c_a, s_a_prime, 1))
            x_b_recon = br.run(1, lambda: self._dec(c_b, s_b_prime, 2))
            if self.guided == 0:
                s_a_use, s_b_use = s_a.to(dev), s_b.to(dev)
                if overlap:
                    # The MLP passes over the sampled styles have no hooked tensor downstream: without a gradient of their own
                    # the exchange's stage 1 would rely on the autograd engine running them before the first decodes' nodes (it
                    # does -- higher sequence numbers first -- but that is an implementation detail).  With requires_grad the
                    # styles' gradients are formed at the END of those MLP passes' backward and stage 1 waits for them.  Costs a
                    # (B, style_dim) backward-data; no parameter gradient changes.
                    s_a_use.requires_grad_(True)
                    s_b_use.requires_grad_(True)
            elif self.guided == 1:
                s_a_use, s_b_use = s_a_prime, s_b_prime
            else:
                raise ValueError("self.guided unknown value: %r" % (self.guided,))
            br.share(c_a, c_b, s_a_use, s_b_use)
            sr_a = sr_b = None
            if fool_sr:
                # the fooling term (trainer.py:521-525) on the step's own codes; the classifiers' weight gradients would be
                # zeroed unused by domain_classifier_sr_update (trainer.py:1241): only the codes' gradients are formed
                # data parallel: the batch norms' statistics span the ranks; their backward exchanges are issued from inside
                # the generator's backward, between the staged all-reduces of GradExchange -- all from the host in the
                # engine's order, the same on every rank
                with ops.bn_world(self._bn_world(hp)):
                    sr_a = br.run(0, lambda: ops.mse_const(self.domain_classifier_sr_a(c_a, False), 0.5))
                    sr_b = br.run(1, lambda: ops.mse_const(self.domain_classifier_sr_b(c_b, False), 0.5))
            if reuse:
                x_ba, x_ab = x_ba_kept, x_ab_kept
            else:
                x_ba = br.run(0, lambda: self._dec(c_b, s_a_use, 1))
                x_ab = br.run(1, lambda: self._dec(c_a, s_b_use, 2))
            # adversarial terms (trainer.py:515-516), issued as soon as the translations exist.  (Giving the two
            # discriminators streams of their own, so that their small grids run beside the encoder / decoder kernels
            # that follow, measured 161.0-161.4 ms per step against 159.9-160.2 on the branch streams: not kept.)
            self.loss_gen_adv_a = br.run(0, lambda: self.dis_a.calc_gen_loss(x_ba))
            self.loss_gen_adv_b = br.run(1, lambda: self.dis_b.calc_gen_loss(x_ab))
            osr_a = osr_b = None
            if fool_out:   # the output classifiers' fooling term (trainer.py:527-532) on the same translations
                osr_a = br.run(0, lambda: self.output_classifier_sr_a.calc_gen_loss_sr(x_ba))
                osr_b = br.run(1, lambda: self.output_classifier_sr_b.calc_gen_loss_sr(x_ab))
            c_b_recon, s_a_recon = br.run(0, lambda: self._enc(x_ba, 1))
            c_a_recon, s_b_recon = br.run(1, lambda: self._enc(x_ab, 2))
            br.share(c_a_recon, c_b_recon)
            cyc = hp["recon_x_cyc_w"] > 0
            x_aba = br.run(0, lambda: self._dec(c_a_recon, s_a_prime, 1)) if cyc else None
            x_bab = br.run(1, lambda: self._dec(c_b_recon, s_b_prime, 2)) if cyc else None

            self.loss_gen_recon_x_a = br.run(0, lambda: self.recon_criterion(x_a_recon, x_a))
            self.loss_gen_recon_x_b = br.run(1, lambda: self.recon_criterion(x_b_recon, x_b))
            self.loss_gen_recon_s_a = br.run(0, lambda: self.recon_criterion(s_a_recon, s_a_use))
            self.loss_gen_recon_s_b = br.run(1, lambda: self.recon_criterion(s_b_recon, s_b_use))
            self.loss_gen_recon_c_a = br.run(1, lambda: self.recon_criterion(c_a_recon, c_a))
            self.loss_gen_recon_c_b = br.run(0, lambda: self.recon_criterion(c_b_recon, c_b))
            self.loss_gen_recon_synth = 0
            if cyc:
                if self.recon_mask:
                    if mask_a is None or mask_b is None:
                        raise ValueError("recon_mask == 1 needs mask_a and mask_b of shape (B,1,H,W)")
                    self.loss_gen_cycrecon_x_a = br.run(0, lambda: self.recon_criterion_mask(x_aba, x_a, mask_a))
                    self.loss_gen_cycrecon_x_b = br.run(1, lambda: self.recon_criterion_mask(x_bab, x_b, mask_b))
                else:
                    self.loss_gen_cycrecon_x_a = br.run(0, lambda: self.recon_criterion(x_aba, x_a))
                    self.loss_gen_cycrecon_x_b = br.run(1, lambda: self.recon_criterion(x_bab, x_b))
            else:
                self.loss_gen_cycrecon_x_a = 0
                self.loss_gen_cycrecon_x_b = 0
            br.join(self.loss_gen_recon_x_a, self.loss_gen_recon_x_b, self.loss_gen_recon_s_a, self.loss_gen_recon_s_b,
                    self.loss_gen_recon_c_a, self.loss_gen_recon_c_b, self.loss_gen_cycrecon_x_a,
                    self.loss_gen_cycrecon_x_b, self.loss_gen_adv_a, self.loss_gen_adv_b, sr_a, sr_b, osr_a, osr_b)
            self.loss_classifier_sr = ops.scalar_sum([sr_a, sr_b]) if fool_sr else 0
            self.loss_output_classifier_sr = ops.scalar_sum([osr_a, osr_b]) if fool_out else 0
            if pair_term or self.semantic_w or vgg_on:
                br.join(x_ab, x_ba)            # both translations on the caller's stream
            self.loss_gen_vgg_a = self.loss_gen_vgg_b = 0
            if vgg_on:
                # trainer.py:493-502: vgg(x_ba, x_b), vgg(x_ab, x_a); the network runs twice on 2B images, not four times on B
                self.loss_gen_vgg_a, self.loss_gen_vgg_b = vgg_loss(self.vgg, [x_ba, x_ab], [x_b, x_a])
            if pair_term:
                # after the cycle terms: its two L1 sign patterns (x_ab > x_b, x_ba > x_a) are the last of the step
                self.loss_gen_recon_synth = ops.pair_l1(x_a, x_b, x_ab, x_ba)
            self.loss_sem_seg = 0
            if self.semantic_w:
                gt = None if gts is None else self._gt_to_device(gts, dev)
                self.loss_sem_seg = self._semantic_loss(x_a, x_b, x_ab, x_ba, mask_a, mask_b, gt)
        finally:
            for p in d_params:
                p.requires_grad_(True)
        self.domain_adv_loss = 0

        pairs = [(hp["gan_w"], self.loss_gen_adv_a), (hp["gan_w"], self.loss_gen_adv_b),
                 (hp["recon_x_w"], self.loss_gen_recon_x_a), (hp["recon_s_w"], self.loss_gen_recon_s_a),
                 (hp["recon_c_w"], self.loss_gen_recon_c_a), (hp["recon_x_w"], self.loss_gen_recon_x_b),
                 (hp["recon_s_w"], self.loss_gen_recon_s_b), (hp["recon_c_w"], self.loss_gen_recon_c_b)]
        if cyc:
            pairs += [(hp["recon_x_cyc_w"], self.loss_gen_cycrecon_x_a),
                      (hp["recon_x_cyc_w"], self.loss_gen_cycrecon_x_b)]
        if vgg_on:
            pairs += [(hp["vgg_w"], self.loss_gen_vgg_a), (hp["vgg_w"], self.loss_gen_vgg_b)]
        if self.semantic_w:
            pairs.append((hp["semantic_w"], self.loss_sem_seg))
        if pair_term:
            pairs.append((hp["recon_synth_w"], self.loss_gen_recon_synth))
        if fool_sr:
            pairs.append((hp["adaptation"]["adv_lambda"], self.loss_classifier_sr))
        if fool_out:
            pairs.append((hp["adaptation"]["output_adv_lambda"], self.loss_output_classifier_sr))
        self.loss_gen_total = ops.weighted_sum([t.detach() for _, t in pairs], [w for w, _ in pairs])
        live = [(w, t) for w, t in pairs if w != 0 and t.requires_grad]
        xch = None
        if overlap:
            # the decoder / MLP half of the flat gradient is exchanged while the first encodes' backward still runs, the content
            # encoders' residual trunks while their down-sampling and first layers (and the style encoder) still run
            streams = [torch.cuda.current_stream(dev)] if dev.type == "cuda" else []
            if br.enabled:
                streams += list(br.s)
            if dev.type == "cuda" and ops.SIDE_STREAM_WGRAD:
                streams.append(ops._side_stream(dev))
            xch = GradExchange(self.gen_opt.flat_g, world, streams)
            xch.arm(self._early_ranges, [c_a, c_b, s_a_prime, s_b_prime] + ([s_a_use, s_b_use] if self.guided == 0 else []))
            if trunk_a is not None and trunk_b is not None:
                xch.arm(self._trunk_ranges, [trunk_a, trunk_b])
            self.last_exchange = xch     # introspection (tests): which stages fired
        torch.autograd.backward([t for _, t in live], [self._const(w, dev) for w, _ in live])
        br.join()                        # the backward pass ran on the branch streams its nodes were recorded on
        ops.join_side_streams()          # backward-weight kernels run on a side stream
        if xch is not None:
            xch.finish()
        else:
            self._all_reduce_mean(self.gen_opt.flat_g)
        self.gen_opt_step()
        self._log(comet_exp, ("loss_gen_adv_a", "loss_gen_adv_b", "loss_gen_recon_x_a", "loss_gen_recon_s_a",
                              "loss_gen_recon_c_a", "loss_gen_recon_x_b", "loss_gen_recon_s_b",
                              "loss_gen_recon_c_b", "loss_gen_cycrecon_x_a", "loss_gen_cycrecon_x_b",
                              "loss_gen_total") + (("loss_gen_vgg_a", "loss_gen_vgg_b") if vgg_on else ())
                  + (("loss_sem_seg",) if self.semantic_w else ())
                  + (("loss_gen_recon_synth",) if synth else ()) + (("loss_classifier_sr",) if fool_sr else ()))
        if fool_out and comet_exp is not None and self.iterations % 100 == 0:     # trainer.py:612-616
            comet_exp.log_metric("loss_output_classifier_adv_sr", self.loss_output_classifier_sr.cpu().detach())

    # ---- dis_update (trainer.py:1133-1190) ---------------------------------------------
    def dis_update(self, x_a, x_b, hyperparameters, comet_exp=None):
        ops.set_compute(self.precision)
        hp = hyperparameters
        self.dis_opt.zero_grad()               # waits for the last update's step, should it still be in flight (_defer_dis_step)
        s_a = torch.randn(x_a.size(0), self.style_dim, 1, 1)
        s_b = torch.randn(x_b.size(0), self.style_dim, 1, 1)
        dev = x_a.device
        fwd_key = self._fwd_key(x_a, x_b)
        x_a, x_b = ops.nhwc(x_a), ops.nhwc(x_b)
        br = _Branches(dev)
        br.adopt(x_a, x_b)
        keep = self.reuse_dis_forward and self.guided == 1     # guided 0: the two updates draw different styles
        self._fwd_cache = None
        with torch.set_grad_enabled(keep):  # without `keep` the generator graph would never be back-propagated here
            c_a, s_a_prime = br.run(0, lambda: self._enc(x_a, 1))
            c_b, s_b_prime = br.run(1, lambda: self._enc(x_b, 2))
            if self.guided == 0:
                s_a_use, s_b_use = s_a.to(dev), s_b.to(dev)
            elif self.guided == 1:
                s_a_use, s_b_use = s_a_prime, s_b_prime
            else:
                raise ValueError("self.guided unknown value: %r" % (self.guided,))
            br.share(c_a, c_b, s_a_use, s_b_use)
            x_ba = br.run(0, lambda: self._dec(c_b, s_a_use, 1))
            x_ab = br.run(1, lambda: self._dec(c_a, s_b_use, 2))
        if keep:
            self._fwd_cache = (fwd_key, (c_a, s_a_prime, c_b, s_b_prime, x_ba, x_ab))
        self.loss_dis_a = br.run(0, lambda: self.dis_a.calc_dis_loss(x_ba.detach(), x_a))
        self.loss_dis_b = br.run(1, lambda: self.dis_b.calc_dis_loss(x_ab.detach(), x_b))
        br.join(self.loss_dis_a, self.loss_dis_b)
        self.loss_dis_total = ops.weighted_sum([self.loss_dis_a.detach(), self.loss_dis_b.detach()],
                                               [hp["gan_w"], hp["gan_w"]])
        w = self._const(hp["gan_w"], dev)
        torch.autograd.backward([self.loss_dis_a, self.loss_dis_b], [w, w])
        br.join()
        ops.join_side_streams()
        if dp_world() and OVERLAP_EXCHANGE and dev.type == "cuda":
            self._defer_dis_step(dev)
        else:
            self._all_reduce_mean(self.dis_opt.flat_g)
            self.dis_opt_step()
        self._log(comet_exp, ("loss_dis_b", "loss_dis_a"))

    # ---- data parallel: the discriminator exchange beside the next generator forward ---------------------------------
    def _defer_dis_step(self, dev):
        """The all-reduce of the discriminator gradient (66 MB), its 1 / world scale and the discriminator's optimizer step
        (Adam + the refresh of the prepared weight images) are enqueued on the communication stream, behind the backward pass
        that just ended on the caller's stream.  The caller's stream goes on: in the reference's iteration the next thing
        is gen_update (scripts/train.py:182-187), whose first ~15 ms -- two encodes, four decodes -- touch no discriminator
        weight, so the exchange runs beside them.  Whatever reads or writes the discriminators next waits at the optimizer's
        gate (StepGate: the top of MsImageDis.forward, state_dict / load_state_dict, apply, every method of the optimizer)."""
        self.dis_opt.step_on(comm_stream(dev), before=lambda: self._all_reduce_mean(self.dis_opt.flat_g),
                             step=self.dis_opt_step)

    def _fwd_key(self, x_a, x_b):
        """Identity of a generator forward: the input tensors (storage, layout, in-place version) and the state of the
        generator weights (optimizer step count and the parameters' in-place versions)."""
        gp = self.gen_opt._plist
        return (x_a.data_ptr(), x_a._version, tuple(x_a.shape), tuple(x_a.stride()), x_b.data_ptr(), x_b._version,
                tuple(x_b.shape), tuple(x_b.stride()), self.gen_opt._step, self.gen_opt.flat_p.data_ptr(),
                sum(p._version for p in gp), self.training, ops.get_compute())

    def _log(self, comet_exp, names):
        if comet_exp is not None and self.iterations % 100 == 0:
            for n in names:
                v = getattr(self, n)
                comet_exp.log_metric(n, v.cpu().detach() if torch.is_tensor(v) else v)

    # ---- schedule (trainer.py:1326-1335) ------------------------------------------------
    def update_learning_rate(self):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # scheduler-before-optimizer order is the reference's (train.py:172)
            if self.dis_scheduler is not None:
                self.dis_scheduler.step()
            if self.gen_scheduler is not None:
                self.gen_scheduler.step()

    # ---- sampling (trainer.py:773-928, core outputs only) -------------------------------
    def sample_fid(self, x_a, x_b):
        """trainer.py:1087-1131: per-sample cross-domain translation a -> b with the style encoded from x_b
        (guided == 1); returns x_ab1 (trainer.py:1126-1131)."""
        ops.set_compute(self.precision)
        self.eval()
        x_ab1 = []
        with torch.no_grad():
            for i in range(x_a.size(0)):
                c_a, _ = self._enc(x_a[i:i + 1], 1)
                _, s_b_fake = self._enc(x_b[i:i + 1], 2)
                if self.guided == 1:
                    x_ab1.append(self._dec(c_a, s_b_fake, 2))
                else:
                    print("self.guided unknown value:", self.guided)
        x_ab1 = torch.cat(x_ab1)
        self.train()
        return x_ab1

    def sample(self, x_a, x_b):
        ops.set_compute(self.precision)
        self.eval()
        outs = [[] for _ in range(6)]
        with torch.no_grad():
            s_a1, s_b1 = self.s_a.to(x_a.device), self.s_b.to(x_a.device)
            s_a2 = torch.randn(x_a.size(0), self.style_dim, 1, 1).to(x_a.device)
            s_b2 = torch.randn(x_b.size(0), self.style_dim, 1, 1).to(x_a.device)
            for i in range(x_a.size(0)):
                xa, xb = x_a[i:i + 1], x_b[i:i + 1]
                c_a, s_a_fake = self._enc(xa, 1)
                c_b, s_b_fake = self._enc(xb, 2)
                outs[0].append(self._dec(c_a, s_a_fake, 1))
                outs[1].append(self._dec(c_b, s_b_fake, 2))
                if self.guided == 0:
                    outs[2].append(self._dec(c_b, s_a1[i:i + 1], 1))
                    outs[3].append(self._dec(c_b, s_a2[i:i + 1], 1))
                    outs[4].append(self._dec(c_a, s_b1[i:i + 1], 2))
                    outs[5].append(self._dec(c_a, s_b2[i:i + 1], 2))
                else:
                    outs[2].append(self._dec(c_b, s_a_fake, 1))
                    outs[3].append(self._dec(c_b, s_a_fake, 1))
                    outs[4].append(self._dec(c_a, s_b_fake, 2))
                    outs[5].append(self._dec(c_a, s_b_fake, 2))
        x_a_recon, x_b_recon, x_ba1, x_ba2, x_ab1, x_ab2 = (torch.cat(o) for o in outs)
        self.train()
        if self.semantic_w:
            self.segmentation_model.eval()
            # colour-coded label maps of the originals and the first translations (trainer.py:854-925)
            with torch.no_grad():
                seg = self.segmentation_model
                rgb_a, rgb_b = colorize(ops.seg_labels(seg(x_a, x_b))).split(x_a.size(0))
                rgb_ab, rgb_ba = colorize(ops.seg_labels(seg(x_ab1, x_ba1))).split(x_a.size(0))
            return x_a, x_a_recon, rgb_a, x_ab1, rgb_ab, x_ab2, x_b, x_b_recon, rgb_b, x_ba1, rgb_ba, x_ba2
        return x_a, x_a_recon, x_ab1, x_ab2, x_b, x_b_recon, x_ba1, x_ba2

    def sample_syn(self, x_a, x_b):
        """trainer.py:930-1085: line for line the body of `sample` under a second name (for synthetic-domain pairs)."""
        return self.sample(x_a, x_b)

    # ---- checkpoints (trainer.py:1337-1429) ---------------------------------------------
    @staticmethod
    def _plain(sd):
        return {k: v.detach().clone(memory_format=torch.contiguous_format).cpu() for k, v in sd.items()}

    def save(self, snapshot_dir, iterations):
        gen_name = os.path.join(snapshot_dir, "gen_%08d.pt" % (iterations + 1))
        dis_name = os.path.join(snapshot_dir, "dis_%08d.pt" % (iterations + 1))
        opt_name = os.path.join(snapshot_dir, "optimizer.pt")
        if self.gen_state == 0:
            torch.save({"a": self._plain(self.gen_a.state_dict()), "b": self._plain(self.gen_b.state_dict())},
                       gen_name)
        else:
            torch.save({"2": self._plain(self.gen.state_dict())}, gen_name)
        torch.save({"a": self._plain(self.dis_a.state_dict()), "b": self._plain(self.dis_b.state_dict())}, dis_name)
        torch.save({"gen": self.gen_opt.state_dict(), "dis": self.dis_opt.state_dict()}, opt_name)

    def resume(self, checkpoint_dir, hyperparameters):
        last_model_name = get_model_list(checkpoint_dir, "gen")
        state_dict = torch.load(last_model_name, map_location="cpu", weights_only=True)
        if self.gen_state == 0:
            self.gen_a.load_state_dict(state_dict["a"])
            self.gen_b.load_state_dict(state_dict["b"])
        else:
            self.gen.load_state_dict(state_dict["2"])
        iterations = int(last_model_name[-11:-3])
        last_model_name = get_model_list(checkpoint_dir, "dis")
        state_dict = torch.load(last_model_name, map_location="cpu", weights_only=True)
        self.dis_a.load_state_dict(state_dict["a"])
        self.dis_b.load_state_dict(state_dict["b"])
        state_dict = torch.load(os.path.join(checkpoint_dir, "optimizer.pt"), map_location="cpu", weights_only=True)
        self.dis_opt.load_state_dict(state_dict["dis"])
        self.gen_opt.load_state_dict(state_dict["gen"])
        self.dis_scheduler = get_scheduler(self.dis_opt, hyperparameters, iterations)
        self.gen_scheduler = get_scheduler(self.gen_opt, hyperparameters, iterations)
        self.gen_opt.invalidate_prepared()      # whatever wrote the weights, the prepared images follow them
        self.dis_opt.invalidate_prepared()
        print("Resume from iteration %d" % iterations)
        return iterations
