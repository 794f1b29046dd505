"""GPU tests of the data-parallel adaptation terms (adaptation.data_parallel: 1).

Kernel level, one process: W ranks are W equal row blocks of one tensor; the local halves of munit_batchnorm_dp_* run once
per block into the block's row of an exchange buffer, the test sums the one-hot buffers itself (what the all-reduce does)
and the finishing halves run per block -- against fp64 batch norm of the WHOLE tensor, under the bounds of
tests/test_gpu_featda.test_batchnorm_against_fp64 (forward tensors and statistics 1e-5, gradients 5e-5 normalised maximum
error), plus the guard-band contract of tests/kernel_contract.py.

Trainer level, two gloo ranks sharing cuda:0 (the pattern of tests/test_gpu_dp.py), batch 1 per rank: with per-rank
statistics every spatially constant channel would normalise to 0 and every gradient would differ, so these cannot pass with
local batch norm.  The collectives carry a 60 s timeout: a mismatched sequence raises instead of hanging."""
import os
import sys
from ctypes import c_float, c_void_p

import pytest
import torch

from munit_amd import _lib
from tests import featda_oracle as D
from tests.conv_contract import ERR_WORKSPACE, GUARD_BYTE, Arena, fill_random, no_nan, poison, stream
from tests.kernel_contract import ERR_ARG, refused
from tests.parity import nerr, pinned, record
from tests.test_gpu_featda import FWD_TOL, GRAD_TOL, LOSS_TOL, _bn_ref, _contract, _rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, MOM = 1e-5, 0.1
# (W, R_local, C): all variance between the ranks (the per-rank batch-1 case); a single partial block; rows that are no
# multiple of the block's row lanes with more than one partial block; several partial blocks; a channel mean of 100 against
# unit spread (the two-float mean and the merge); C > 256, where the row, combine and finish kernels (one thread per
# channel) run over several blocks: C = 1024 at one row lane (4 blocks), and C = 512 (2 blocks) with 3 partial blocks of 11 rows
CASES = [(2, 1, 4), (2, 7, 64), (3, 257, 128), (2, 1024, 64), (4, 33, 128), (2, 5, 1024), (3, 33, 512)]


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


class _Blocks(object):
    """W row blocks of one (W * R, C) tensor and the per-rank state of a cross-rank batch norm."""

    def __init__(self, w, r, c, relu, mean=0.0, seed=1):
        self.lib = _lib.load()
        self.w, self.r, self.c, self.relu = w, r, c, relu
        self.x, self.dy = _rows(w * r, c, seed, mean), _rows(w * r, c, seed + 1)
        g = torch.Generator().manual_seed(seed + 2)
        self.gamma, self.beta = 1 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
        self.xd, self.dyd = self.x.to(DEV), self.dy.to(DEV)
        self.gd, self.bd = self.gamma.to(DEV), self.beta.to(DEV)
        self.nws = self.lib.munit_batchnorm_dp_workspace_bytes(c)
        self.ws = torch.empty(self.nws, dtype=torch.uint8, device=DEV)
        self.rm = [torch.zeros(c, device=DEV) for _ in range(w)]
        self.rv = [torch.ones(c, device=DEV) for _ in range(w)]

    def blk(self, t, k):
        return t[k * self.r:(k + 1) * self.r]

    def forward(self, combine_w=None):
        """local statistics per block, the sum of the one-hot buffers, combine + apply per block"""
        lib, w, r, c = self.lib, self.w, self.r, self.c
        rows = []
        for k in range(w):
            xch = torch.full((w * 3 * c,), float("nan"), device=DEV)
            _lib.check(lib.munit_batchnorm_dp_stats_local(_p(self.blk(self.xd, k)), r, c, w, k, _p(xch), xch.numel(),
                                                          _p(self.ws), self.nws, stream()), "stats_local")
            other = torch.ones(w, dtype=torch.bool)
            other[k] = False
            assert bool((xch.view(w, 3 * c)[other.to(DEV)] == 0).all())            # one-hot: the other rows are zero
            rows.append(xch)
        self.xch_f = torch.stack(rows).sum(0)
        assert torch.equal(self.xch_f.view(w, 3 * c), torch.stack([rows[k].view(w, 3 * c)[k] for k in range(w)]))
        wc = combine_w or w
        self.y = torch.empty_like(self.xd)
        self.mean = [torch.empty(2 * c, device=DEV) for _ in range(w)]
        self.rstd = [torch.empty(2 * c, device=DEV) for _ in range(w)]       # high parts, low parts
        for k in range(wc):
            _lib.check(lib.munit_batchnorm_dp_fwd_apply(_p(self.blk(self.xd, k)), _p(self.blk(self.y, k)), _p(self.mean[k]),
                                                        _p(self.rstd[k]), _p(self.rm[k]), _p(self.rv[k]), r, c, wc,
                                                        _p(self.xch_f), self.xch_f.numel(), _p(self.gd), _p(self.bd),
                                                        self.relu, c_float(EPS), c_float(MOM), stream()), "fwd_apply")
        torch.cuda.synchronize()

    def backward(self, acc=0.0, with_w=True, fill=7.0):
        lib, w, r, c = self.lib, self.w, self.r, self.c
        rows = []
        for k in range(w):
            xch = torch.full((w * 4 * c,), float("nan"), device=DEV)
            _lib.check(lib.munit_batchnorm_dp_bwd_local(_p(self.blk(self.xd, k)), _p(self.blk(self.dyd, k)),
                                                        _p(self.blk(self.y, k)), _p(self.mean[k]), _p(self.rstd[k]), r, c,
                                                        self.relu, w, k, _p(xch), xch.numel(), _p(self.ws), self.nws,
                                                        stream()), "bwd_local")
            rows.append(xch)
        xch = torch.stack(rows).sum(0)
        dx = torch.empty_like(self.xd)
        dg = [torch.full((c,), fill, device=DEV) for _ in range(w)]
        db = [torch.full((c,), fill, device=DEV) for _ in range(w)]
        for k in range(w):
            _lib.check(lib.munit_batchnorm_dp_bwd_finish(_p(self.blk(self.xd, k)), _p(self.blk(self.dyd, k)),
                                                         _p(self.blk(self.y, k)), _p(self.gd), _p(self.mean[k]),
                                                         _p(self.rstd[k]), _p(self.blk(dx, k)), _p(dg[k]) if with_w else None,
                                                         _p(db[k]) if with_w else None, c_float(acc), r, c, self.relu, w, k,
                                                         _p(xch), xch.numel(), _p(self.ws), self.nws, stream()), "bwd_finish")
        torch.cuda.synchronize()
        return dx, dg, db


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wrc", CASES)
def test_cross_rank_batchnorm_against_fp64_of_the_whole_tensor(wrc, relu):
    """Forward and backward at every (W, R_local, C) under the bounds of test_gpu_featda.test_batchnorm_against_fp64.

    (2, 1, 4) is the hard one for `dx`: with N = 2 rows per channel xhat is +-1 / sqrt(1 + eps / var), so g - mean(g) and
    xhat * mean(g * xhat) cancel to eps / var of their size (max |dx| 4.0e-3 against max |dy| 3.0), and one fp32 rounding of
    xhat, rstd or a sum (6e-8) becomes 1e-4 of the result -- which is why the cross-rank backward carries rstd and the
    exchanged sums as two floats each and forms dx in double."""
    w, r, c = wrc
    b = _Blocks(w, r, c, relu, mean=100.0 if wrc == (4, 33, 128) else 0.0)
    ry, rm_, rrstd, runb, rdx, rdg, rdb = _bn_ref(b.x, b.gamma, b.beta, relu, b.dy)
    b.forward()
    y, m, rstd = b.y, b.mean[0], b.rstd[0][:c].double() + b.rstd[0][c:].double()
    dx, dg, db = b.backward()
    dg_sum = torch.stack([t.double().cpu() for t in dg]).sum(0)
    db_sum = torch.stack([t.double().cpu() for t in db]).sum(0)
    errs = dict(y=nerr(y, ry), mean=nerr(m[:c].double() + m[c:].double(), rm_), rstd=nerr(rstd, rrstd), dx=nerr(dx, rdx),
                dgamma=nerr(dg_sum, rdg), dbeta=nerr(db_sum, rdb))
    print("cross-rank batchnorm", wrc, relu, errs)
    if relu:                                            # a y within rounding of 0 may sit on the other side of the kink
        near = (ry.abs() < 1e-5 * float(ry.abs().max())) & ((y.cpu() > 0) != (ry > 0))
        assert int(near.sum()) == int(((y.cpu() > 0) != (ry > 0)).sum())
    for k in ("y", "mean", "rstd"):
        assert errs[k] <= FWD_TOL, errs
    for k in ("dx", "dgamma", "dbeta"):
        assert errs[k] <= GRAD_TOL, errs
    # rank symmetry: whichever block is a rank's own, the merged statistics are bitwise the same
    for k in range(1, w):
        assert torch.equal(b.mean[k], b.mean[0]) and torch.equal(b.rstd[k], b.rstd[0])
        assert torch.equal(b.rm[k], b.rm[0]) and torch.equal(b.rv[k], b.rv[0])
    # the running statistics after two calls: momentum 0.1, unbiased variance of the joined batch
    y1 = y.clone()
    b.forward()
    assert torch.equal(b.y, y1)
    assert nerr(b.rm[0], 0.19 * rm_) <= FWD_TOL and nerr(b.rv[0], 0.81 + 0.19 * runb) <= FWD_TOL, \
        (nerr(b.rm[0], 0.19 * rm_), nerr(b.rv[0], 0.81 + 0.19 * runb))
    for k in range(1, w):
        assert torch.equal(b.rm[k], b.rm[0]) and torch.equal(b.rv[k], b.rv[0])
    # a second backward is bitwise the first; acc = 1 accumulates the LOCAL sums; null dgamma / dbeta form dx only
    dx2, dg2, db2 = b.backward()
    assert torch.equal(dx2, dx) and all(torch.equal(u, v) for u, v in zip(dg + db, dg2 + db2))
    dx3, dg3, db3 = b.backward(acc=1.0)
    assert torch.equal(dx3, dx)
    for k in range(w):
        assert torch.equal(dg3[k], 7.0 + dg[k]) and torch.equal(db3[k], 7.0 + db[k])
    dx4, dg4, db4 = b.backward(with_w=False)
    assert torch.equal(dx4, dx) and all(bool((t == 7.0).all()) for t in dg4 + db4)


def test_a_combine_over_one_rank_is_not_the_joined_batch():
    """The witness that the comparison tells cross-rank statistics from per-rank ones: at (2, 1, 4) a rank's own row holds
    M2 = 0, so merging W = 1 rows gives rstd = 1 / sqrt(eps) -- far from the joined batch's."""
    b = _Blocks(2, 1, 4, 0)
    _, _, rrstd, _, _, _, _ = _bn_ref(b.x, b.gamma, b.beta, 0, b.dy)
    b.forward()
    joined = b.rstd[0][:4].clone()
    assert nerr(joined, rrstd) <= FWD_TOL
    b.forward(combine_w=1)
    alone = float(1.0 / torch.sqrt(torch.tensor(EPS, dtype=torch.float32).double()))
    assert bool((b.rstd[0][:4] == torch.tensor(alone).float().item()).all()), b.rstd[0]
    assert float((b.rstd[0][:4].cpu().double() / rrstd).min()) > 10.0


@pytest.mark.parametrize("wrc", [(2, 7, 64), (3, 257, 128), (2, 5, 1024)])
def test_guard_bands_cross_rank_batchnorm(wrc):
    lib = _lib.load()
    w, r, c = wrc
    rank = w - 1
    n, nws = r * c * 4, lib.munit_batchnorm_dp_workspace_bytes(c)
    n3, n2 = w * 3 * c, w * 4 * c
    a = Arena(dict(x=n, dy=n, gamma=c * 4, beta=c * 4, rm=c * 4, rv=c * 4, y=n, mean=c * 8, rstd=c * 8, dx=n, dg=c * 4,
                   db=c * 4, xch3=n3 * 4, xch2=n2 * 4, ws=nws), torch.device(DEV))
    for i, nm in enumerate(("x", "dy", "gamma", "beta")):
        fill_random(a.view(nm, torch.float32), 80 + i)
    p = a.ptr

    def reset_running():
        a.view("rm", torch.float32).fill_(0.25)
        a.view("rv", torch.float32).fill_(1.5)

    def stats(x="x", w_=w, c_=c, floats=n3, ws_bytes=nws):
        return lib.munit_batchnorm_dp_stats_local(p(x) if x else None, r, c_, w_, rank if w_ else 0, p("xch3"), floats,
                                                  p("ws"), ws_bytes, stream())

    def apply(x="x", w_=w, c_=c, floats=n3):
        reset_running()
        return lib.munit_batchnorm_dp_fwd_apply(p(x) if x else None, p("y"), p("mean"), p("rstd"), p("rm"), p("rv"), r, c_, w_,
                                                p("xch3"), floats, p("gamma"), p("beta"), 1, c_float(EPS), c_float(MOM),
                                                stream())

    def blocal(x="x", w_=w, c_=c, floats=n2, ws_bytes=nws):
        return lib.munit_batchnorm_dp_bwd_local(p(x) if x else None, p("dy"), p("y"), p("mean"), p("rstd"), r, c_, 1, w_,
                                                rank if w_ else 0, p("xch2"), floats, p("ws"), ws_bytes, stream())

    def bfinish(x="x", w_=w, c_=c, floats=n2, ws_bytes=nws):
        return lib.munit_batchnorm_dp_bwd_finish(p(x) if x else None, p("dy"), p("y"), p("gamma"), p("mean"), p("rstd"),
                                                 p("dx"), p("dg"), p("db"), c_float(0.0), r, c_, 1, w_, rank if w_ else 0,
                                                 p("xch2"), floats, p("ws"), ws_bytes, stream())

    def refusals(L, call, outs, short_ws=True):
        cases = [("x = NULL", lambda: call(x=None), ERR_ARG), ("W = 0", lambda: call(w_=0), ERR_ARG),
                 ("C = 6", lambda: call(c_=6), ERR_ARG), ("exchange buffer one float short", lambda: call(floats=call.floats - 1),
                                                         ERR_ARG)]
        if short_ws:
            cases.append(("workspace one byte short", lambda: call(ws_bytes=nws - 1), ERR_WORKSPACE))
        for label, fn, code in cases:
            for o in outs:
                poison(a.view(o, torch.float32), 0)
            a.bytes("ws").fill_(GUARD_BYTE)
            refused(L, fn(), outs, label, code=code)

    stats.floats, apply.floats, blocal.floats, bfinish.floats = n3, n3, n2, n2
    what = "batchnorm_dp %s" % (wrc,)
    # the local half of the forward writes the whole exchange buffer (its own row and the zeros)
    L = _contract(a, ["x", "dy", "gamma", "beta"], ["xch3"], what + " stats_local", stats)
    refusals(L, stats, ["xch3"])
    _lib.check(stats(), "stats_local")
    torch.cuda.synchronize()
    rows = a.view("xch3", torch.float32).view(w, 3 * c)
    assert bool((rows[:rank] == 0).all()) and bool((rows[rank, 2 * c:] > 0).all())
    # combine + apply on the buffer as one rank left it (the other rows zero): no workspace
    L = _contract(a, ["x", "dy", "gamma", "beta", "xch3"], ["y", "mean", "rstd"], what + " fwd_apply", apply)
    assert no_nan(a.view("rm", torch.float32)) and no_nan(a.view("rv", torch.float32))
    refusals(L, apply, ["y", "mean", "rstd"], short_ws=False)
    assert bool((a.view("rm", torch.float32) == 0.25).all()) and bool((a.view("rv", torch.float32) == 1.5).all())
    _lib.check(apply(), "fwd_apply")
    L = _contract(a, ["x", "dy", "gamma", "y", "mean", "rstd"], ["xch2"], what + " bwd_local", blocal)
    refusals(L, blocal, ["xch2"])
    _lib.check(blocal(), "bwd_local")
    torch.cuda.synchronize()
    assert bool((a.view("xch2", torch.float32).view(w, 4 * c)[:rank] == 0).all())
    L = _contract(a, ["x", "dy", "gamma", "y", "mean", "rstd", "xch2"], ["dx", "dg", "db"], what + " bwd_finish", bfinish)
    refusals(L, bfinish, ["dx", "dg", "db"])


# ---- two gloo ranks on cuda:0 ---------------------------------------------------------------------------------------------
def _init(rank, world, tmpdir, tag, no_overlap=False):
    import datetime
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from munit_amd import trainer as T
    # MUNIT_NO_OVERLAP_EXCHANGE is read once, when munit_amd.trainer is imported -- which unpickling this worker has already
    # done: the parent sets the variable before it spawns the ranks
    assert T.OVERLAP_EXCHANGE == (not no_overlap)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(tmpdir, "rdzv_" + tag), rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    return T, dist


def _cpu_state(mod):
    return {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}


def _feat_hp(batch):
    from oracle import munit_oracle as O
    hp = O.default_hp(256, batch, 1)
    hp["gen"]["n_res"] = 1
    hp["dis"]["num_scales"] = 1
    hp["adaptation"].update(adv_lambda=6, dfeat_lambda=1, data_parallel=1)
    return hp


def _feat_worker(rank, world, tmpdir, no_overlap):
    from munit_amd import ops
    from oracle import munit_oracle as O
    T, dist = _init(rank, world, tmpdir, "feat%d" % no_overlap, no_overlap)
    dev = torch.device(DEV)
    hp = _feat_hp(1)
    torch.manual_seed(0)                            # the ranks start from the same weights: same seed, as bench.py's ranks do
    tr = T.MUNIT_Trainer(dict(hp)).to(dev)
    x_a, x_b, m_a, m_b = [t[rank:rank + 1].to(dev) for t in O.synthetic_batch(2, 256)]
    out = {"updates": []}

    def codes():
        with torch.no_grad():
            return (tr._content_enc(1)(ops.nhwc(x_a)).cpu().double(), tr._content_enc(2)(ops.nhwc(x_b)).cpu().double())

    def recorded(fn):
        return [t.cpu() for t in record(fn, mask=None, l1=None, dann=True)[2].dann]

    for it, synth in ((0, False), (1, True)):
        rec = {"sd_a": _cpu_state(tr.domain_classifier_sr_a), "sd_b": _cpu_state(tr.domain_classifier_sr_b), "codes": codes(),
               "synth": synth}
        rec["sink"] = recorded(lambda: tr.domain_classifier_sr_update(x_a, x_b, synth, 1.0, it))
        rec["loss"] = float(tr.loss_classifier_sr_update)
        rec["grads"] = [p._munit_grad.detach().cpu().clone(memory_format=torch.contiguous_format)
                        for p in tr.classif_opt_sr._plist]
        out["updates"].append(rec)
    torch.manual_seed(11)
    tr.dis_update(x_a, x_b, hp)
    out["fool"] = {"sd_a": _cpu_state(tr.domain_classifier_sr_a), "sd_b": _cpu_state(tr.domain_classifier_sr_b),
                   "codes": codes()}
    _, km, k = record(lambda: tr.gen_update(x_a, x_b, hp, m_a, m_b), dann=True)
    out["fool"]["sink"], out["fool"]["kinks"] = [t.cpu() for t in k.dann], (km.masks, km.l1_signs)
    out["fool"]["loss"] = float(tr.loss_classifier_sr.detach())
    if not no_overlap:
        assert tr.last_exchange is not None and tr.last_exchange.fired      # the staged exchange ran inside backward
    out["classif_p"] = tr.classif_opt_sr.flat_p.detach().cpu().clone()
    out["gen_p"] = tr.gen_opt.flat_p.detach().cpu().clone()
    out["gen_g"] = tr.gen_opt.flat_g.detach().cpu().clone()
    out["dis_p"] = tr.dis_opt.flat_p.detach().cpu().clone()        # read after gen_update: the step may have been deferred
    out["sd_a"], out["sd_b"] = _cpu_state(tr.domain_classifier_sr_a), _cpu_state(tr.domain_classifier_sr_b)
    torch.save(out, os.path.join(tmpdir, "feat%d_rank%d.pt" % (no_overlap, rank)))
    dist.barrier()
    dist.destroy_process_group()


def _oracle_state(sd):
    return {k: (v.long() if k.endswith("tracked") else v.double().clone()) for k, v in sd.items()}


def _joint_pins(r0, r1):
    assert len(r0) == len(r1) == 2 * D.PINS_PER_CALL
    return D.trainer_pins([torch.cat([u, v], 0) for u, v in zip(r0, r1)])


def _generator_gradient_check(hp2, orc_cls, r0, r1, joint, kinks0, kinks1, attach=None):
    """The ranks' averaged generator gradient (r0["gen_g"], bitwise r1's) against the fp64 oracle's gen_update on the JOINED
    batch -- the scheme of test_gpu_dp.test_two_rank_step_matches_the_oracle_on_the_joint_batch: a trainer built under the
    ranks' seed hosts the per-tensor views and hands the oracle the initial generator; the discriminators are the ones the
    ranks' gen_update saw; each rank's ReLU / LeakyReLU / L1 branches are concatenated along the batch axis.  Bounds:
    tests/parity.GradCheck's pinned ones."""
    from munit_amd.trainer import MUNIT_Trainer
    from oracle import munit_oracle as O
    from tests.parity import GradCheck, oracle_states, trainer_named_params
    torch.manual_seed(0)
    tr = MUNIT_Trainer(dict(hp2)).to(DEV)
    gnames, dnames = trainer_named_params(tr)
    orc = orc_cls(dict(hp2), *oracle_states(hp2, torch.float64))
    if attach is not None:
        orc.attach(*attach)
    with torch.no_grad():
        tr.dis_opt.flat_p.copy_(r0["dis_p"].to(DEV))
        for (n, p), q in list(zip(gnames, orc.opt["gen"]["params"])) + list(zip(dnames, orc.opt["dis"]["params"])):
            q.copy_(p.detach().double().cpu())
    (m0, s0), (m1, s1) = kinks0, kinks1
    assert len(m0) == len(m1) > 0 and len(s0) == len(s1)
    km = O.KinkMasks([torch.cat([a, b], 0) for a, b in zip(m0, m1)], [torch.cat([a, b], 0) for a, b in zip(s0, s1)])
    with pinned(km, "gen_update on the joint batch"):
        g_ref = orc.gen_update(*joint)
    tr.gen_opt.flat_g.copy_(r0["gen_g"].to(DEV))
    gc, n_checked = GradCheck(pinned=True), 0
    for (n, p), g in zip(gnames, g_ref):
        if g is None or float(g.abs().max()) < 1e-7:             # a conv bias ahead of an instance norm / AdaIN
            continue
        gc.add("gen." + n, p._munit_grad, g)
        n_checked += 1
    gc.finish()
    assert n_checked >= 40, n_checked
    return orc, gc, n_checked


def _spawn(worker, tmp_path, monkeypatch, no_overlap, *args):
    import torch.multiprocessing as mp
    if no_overlap:
        monkeypatch.setenv("MUNIT_NO_OVERLAP_EXCHANGE", "1")
    else:
        monkeypatch.delenv("MUNIT_NO_OVERLAP_EXCHANGE", raising=False)
    mp.spawn(worker, args=(2, str(tmp_path)) + args + (no_overlap,), nprocs=2, join=True)


def test_two_rank_feature_level_updates_match_the_oracle_on_the_joined_batch(tmp_path, monkeypatch):
    """domain_classifier_sr_update on real images, on synthetic images, then dis_update + gen_update, batch 1 per rank,
    adv_lambda 6 / dfeat_lambda 1 / data_parallel 1 at crop 256: both ranks end with bitwise equal classifier weights,
    batch-norm buffers and generator weights; the averaged classifier gradient of each update against tests/featda_oracle.py
    on the JOINED batch of 2 (the kinks of both ranks concatenated along the batch axis, tests/parity.GradCheck's pinned
    bounds), the update's loss and gen_update's fooling loss -- means over the ranks -- within 1e-5 relative of the joined
    batch's; the averaged GENERATOR gradient of gen_update against the full fp64 step oracle with the fooling term on the
    joined batch (_generator_gradient_check); once with the staged generator exchange and once with MUNIT_NO_OVERLAP_EXCHANGE=1, which agree bitwise."""
    from tests.parity import GradCheck
    runs = {}
    for no_overlap in (0, 1):
        _spawn(_feat_worker, tmp_path, monkeypatch, no_overlap)
        r = [torch.load(tmp_path / ("feat%d_rank%d.pt" % (no_overlap, k)), weights_only=True) for k in range(2)]
        for key in ("classif_p", "gen_p", "gen_g"):
            assert torch.equal(r[0][key], r[1][key]), (no_overlap, key)
        for sd in ("sd_a", "sd_b"):
            for k in r[0][sd]:
                assert torch.equal(r[0][sd][k], r[1][sd][k]), (no_overlap, sd, k)
        runs[no_overlap] = r
    for key in ("classif_p", "gen_p", "gen_g"):                  # staged and serial exchange: the same bits
        assert torch.equal(runs[0][0][key], runs[1][0][key]), key
    r0, r1 = runs[0]
    assert float(r0["gen_g"].abs().max()) > 0
    names = ["a." + n for n in D.param_names()] + ["b." + n for n in D.param_names()]
    for u0, u1 in zip(r0["updates"], r1["updates"]):
        for k in u0["sd_a"]:                                     # both ranks entered the update with the same classifiers
            assert torch.equal(u0["sd_a"][k], u1["sd_a"][k]) and torch.equal(u0["sd_b"][k], u1["sd_b"][k]), k
        sd_a, sd_b = _oracle_state(u0["sd_a"]), _oracle_state(u0["sd_b"])
        ps = D.params(sd_a) + D.params(sd_b)
        for p in ps:
            p.requires_grad_(True)
        c_a, c_b = torch.cat([u0["codes"][0], u1["codes"][0]]), torch.cat([u0["codes"][1], u1["codes"][1]])
        pins = _joint_pins(u0["sink"], u1["sink"])
        loss = D.sr_loss(sd_a, sd_b, c_a, c_b, u0["synth"], False, pins)
        assert pins.done() and pins.worst <= 1e-5, (pins.worst, pins.n_disagree)
        grads = torch.autograd.grad(loss, ps)
        got = 0.5 * (u0["loss"] + u1["loss"])
        rel = abs(got - float(loss.detach())) / abs(float(loss.detach()))
        gc = GradCheck(pinned=True)
        for n, g0, g1, g in zip(names, u0["grads"], u1["grads"], grads):
            assert torch.equal(g0, g1), n                        # the averaged gradient, bitwise the same on both ranks
            gc.add(n, g0, g)
        gc.finish()
        print("two-rank classifier update (synth %s): loss rel %.2e, gradients worst max %.2e L2 %.2e median %.2e"
              % (u0["synth"], rel, gc.worst_max, gc.worst_l2, gc.median))
        assert rel <= LOSS_TOL
    f0, f1 = r0["fool"], r1["fool"]
    sd_a, sd_b = _oracle_state(f0["sd_a"]), _oracle_state(f0["sd_b"])
    c_a, c_b = torch.cat([f0["codes"][0], f1["codes"][0]]), torch.cat([f0["codes"][1], f1["codes"][1]])
    pins = _joint_pins(f0["sink"], f1["sink"])
    l_ref, _, _ = D.fool_term(sd_a, sd_b, c_a, c_b, pins=pins)
    got = 0.5 * (f0["loss"] + f1["loss"])
    rel = abs(got - float(l_ref)) / abs(float(l_ref))
    print("two-rank gen_update: loss_classifier_sr %.6f (mean over the ranks) rel %.2e" % (got, rel))
    assert rel <= LOSS_TOL
    # the averaged generator gradient: the cross-rank backward inside the generator's backward, through to the encoders
    from oracle import munit_oracle as O
    shared = {"sd": (_oracle_state(f0["sd_a"]), _oracle_state(f0["sd_b"])),
              "sink": [torch.cat([u, v], 0) for u, v in zip(f0["sink"], f1["sink"])]}
    joint = [t.double() for t in O.synthetic_batch(2, 256)]
    orc, gc, n = _generator_gradient_check(_feat_hp(2), D.oracle_trainer_class(shared), r0, r1, joint, f0["kinks"], f1["kinks"])
    rel = abs(got - float(orc.losses["loss_classifier_sr"])) / abs(float(orc.losses["loss_classifier_sr"]))
    print("two-rank gen_update: %d generator gradients worst max %.2e L2 %.2e median %.2e, classifier kinks %.2e, loss rel %.2e"
          % (n, gc.worst_max, gc.worst_l2, gc.median, shared["worst"], rel))
    assert shared["worst"] <= 5e-5 and rel <= LOSS_TOL              # tests/parity.KINK_NOISE
    for sd, ref in ((r0["sd_a"], sd_a), (r0["sd_b"], sd_b)):     # the running statistics moved by the joined batch's
        for k, v in ref.items():
            if k.endswith(("running_mean", "running_var")):
                assert nerr(sd[k], v) <= FWD_TOL, (k, nerr(sd[k], v))


# ---- output level ------------------------------------------------------------------------------------------------------------
def _out_hp(batch):
    from oracle import munit_oracle as O
    hp = O.default_hp(64, batch, 1)
    hp["gen"]["n_res"] = 1
    hp["adaptation"].update(output_classifier_lambda=1, output_adv_lambda=1, data_parallel=1)
    return hp


def _out_worker(rank, world, tmpdir, no_overlap):
    from oracle import munit_oracle as O
    T, dist = _init(rank, world, tmpdir, "out", no_overlap)
    dev = torch.device(DEV)
    hp = _out_hp(1)
    torch.manual_seed(0)
    tr = T.MUNIT_Trainer(dict(hp)).to(dev)
    x_a, x_b, m_a, m_b = [t[rank:rank + 1].to(dev) for t in O.synthetic_batch(2, 64, seed=7)]
    x_as, x_bs = [t[rank:rank + 1].to(dev) for t in O.synthetic_batch(2, 64, seed=8)[:2]]
    out = {"sd_a": _cpu_state(tr.output_classifier_sr_a), "sd_b": _cpu_state(tr.output_classifier_sr_b)}
    km = record(lambda: tr.output_domain_classifier_sr_update(x_a, x_as, x_b, x_bs, hp, 0))[1]
    out["masks"] = km.masks
    assert not km.l1_signs
    out["loss"] = float(tr.loss_output_classifier_sr_update)
    out["grads"] = [p._munit_grad.detach().cpu().clone(memory_format=torch.contiguous_format)
                    for p in tr.output_classif_opt_sr._plist]
    out["cls_p"] = tr.output_classif_opt_sr.flat_p.detach().cpu().clone()
    out["sd_a_end"], out["sd_b_end"] = _cpu_state(tr.output_classifier_sr_a), _cpu_state(tr.output_classifier_sr_b)
    torch.manual_seed(11)
    tr.dis_update(x_a, x_b, hp)
    km = record(lambda: tr.gen_update(x_a, x_b, hp, m_a, m_b))[1]
    out["kinks"] = (km.masks, km.l1_signs)
    assert float(tr.loss_output_classifier_sr.detach()) > 0
    out["fool_loss"] = float(tr.loss_output_classifier_sr.detach())
    out["gen_g"] = tr.gen_opt.flat_g.detach().cpu().clone()
    out["gen_p"] = tr.gen_opt.flat_p.detach().cpu().clone()
    out["dis_p"] = tr.dis_opt.flat_p.detach().cpu().clone()
    out["cls_p_end"] = tr.output_classif_opt_sr.flat_p.detach().cpu().clone()
    torch.save(out, os.path.join(tmpdir, "out_rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_output_level_update_matches_the_oracle_on_the_joined_batch(tmp_path, monkeypatch):
    """output_domain_classifier_sr_update, then dis_update + gen_update with the output classifiers' fooling term, batch 1 per
    rank at crop 64: bitwise equal output_classif_opt_sr.flat_p (and generator and discriminator weights) on both ranks, the
    averaged classifier gradient against tests/outda_oracle.py on the joined batch of 2 with both ranks' LeakyReLU branches
    concatenated along the batch axis (tests/parity.GradCheck's pinned bounds), the loss within 1e-5 relative; then the
    averaged generator gradient of gen_update against the fp64 step oracle with the output term on the joined batch."""
    from oracle import munit_oracle as O
    from tests import outda_oracle as U
    from tests.parity import GradCheck
    _spawn(_out_worker, tmp_path, monkeypatch, 0)
    r0, r1 = [torch.load(tmp_path / ("out_rank%d.pt" % k), weights_only=True) for k in range(2)]
    for key in ("cls_p", "gen_p", "gen_g", "dis_p", "cls_p_end"):
        assert torch.equal(r0[key], r1[key]), key
    assert torch.equal(r0["cls_p"], r0["cls_p_end"])            # gen_update forms no classifier step
    hp = _out_hp(2)
    sd_a = {k: v.double().clone() for k, v in r0["sd_a"].items()}
    sd_b = {k: v.double().clone() for k, v in r0["sd_b"].items()}
    for k in sd_a:
        assert torch.equal(r0["sd_a"][k], r1["sd_a"][k]) and torch.equal(r0["sd_b"][k], r1["sd_b"][k]), k
    opt = U.ClassifierOptimizer(sd_a, sd_b, hp)
    x_a, x_b = [t.double() for t in O.synthetic_batch(2, 64, seed=7)[:2]]
    x_as, x_bs = [t.double() for t in O.synthetic_batch(2, 64, seed=8)[:2]]
    assert len(r0["masks"]) == len(r1["masks"]) > 0
    km = O.KinkMasks([torch.cat([u, v], 0) for u, v in zip(r0["masks"], r1["masks"])], [])
    with pinned(km, "output classifier update on the joined batch"):
        loss, grads = U.classifier_update(sd_a, sd_b, opt, x_a, x_as, x_b, x_bs, hp)
    got = 0.5 * (r0["loss"] + r1["loss"])
    rel = abs(got - float(loss)) / abs(float(loss))
    names = ["a." + k for k in sd_a] + ["b." + k for k in sd_b]
    gc = GradCheck(pinned=True)
    n_checked = 0
    for n, g0, g1, g in zip(names, r0["grads"], r1["grads"], grads):
        assert torch.equal(g0, g1), n
        if float(g.abs().max()) < 1e-7:
            continue
        gc.add(n, g0, g)
        n_checked += 1
    gc.finish()
    print("two-rank output classifier update: loss rel %.2e, %d gradients worst max %.2e L2 %.2e median %.2e"
          % (rel, n_checked, gc.worst_max, gc.worst_l2, gc.median))
    assert rel <= LOSS_TOL and n_checked == len(names)
    # the averaged generator gradient of gen_update with the fooling term, on the classifiers the update stepped to
    cls = [{k: v.double().clone() for k, v in r0[key].items()} for key in ("sd_a_end", "sd_b_end")]
    joint = [t.double() for t in O.synthetic_batch(2, 64, seed=7)]
    orc, gc, n = _generator_gradient_check(hp, U.oracle_trainer_class(), r0, r1, joint, r0["kinks"], r1["kinks"], attach=cls)
    got, ref = 0.5 * (r0["fool_loss"] + r1["fool_loss"]), float(orc.losses["loss_output_classifier_sr"])
    print("two-rank gen_update (output level): %d generator gradients worst max %.2e L2 %.2e median %.2e, loss rel %.2e"
          % (n, gc.worst_max, gc.worst_l2, gc.median, abs(got - ref) / abs(ref)))
    assert abs(got - ref) <= LOSS_TOL * abs(ref)


# ---- the reference's Final_test configurations ---------------------------------------------------------------------------------
FINAL_IT = 1        # at tests/final_configs.reduced_hp's cadence the classifier updates fall on it = 1


def _final_hp(name, ckpt, batch):
    from tests import final_configs as C
    hp = C.reduced_hp(C.load(), name, ckpt)
    hp["batch_size"] = batch
    hp["adaptation"]["data_parallel"] = 1
    return hp


def _final_worker(rank, world, tmpdir, name, ckpt, no_overlap):
    from munit_amd import ops
    from tests import final_configs as C
    T, dist = _init(rank, world, tmpdir, "final", no_overlap)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from train_loop import run_iteration
    dev = torch.device(DEV)
    hp = _final_hp(name, ckpt, 1)
    torch.manual_seed(0)
    tr = T.MUNIT_Trainer(dict(hp)).to(dev)
    real, synth = C.inputs(dict(hp, batch_size=2))               # the joined batch; this rank's sample of every tensor
    dreal = tuple(t[rank:rank + 1].to(dev) for t in real)
    dsynth = tuple(t[rank:rank + 1].to(dev) for t in synth[:3]) + tuple(t[rank:rank + 1] for t in synth[3:])
    out = {"calls": [], "losses": {}}

    def pairs():
        while True:
            yield dsynth

    def on_call(method, args, run):
        out["calls"].append(method)
        torch.manual_seed(100 + len(out["calls"]))
        real_cls = method == "domain_classifier_sr_update" and not args[2]
        if real_cls:
            out["sd_a"], out["sd_b"] = _cpu_state(tr.domain_classifier_sr_a), _cpu_state(tr.domain_classifier_sr_b)
            with torch.no_grad():
                out["codes"] = (tr._content_enc(1)(ops.nhwc(args[0])).cpu().double(),
                                tr._content_enc(2)(ops.nhwc(args[1])).cpu().double())
        out_cls = method == "output_domain_classifier_sr_update"
        if out_cls:
            out["sd_a"], out["sd_b"] = _cpu_state(tr.output_classifier_sr_a), _cpu_state(tr.output_classifier_sr_b)
        _, km, k = record(run, mask=out_cls or None, l1=out_cls or None, dann=real_cls or None)
        if real_cls:
            out["sink"] = [t.cpu() for t in k.dann]
        if out_cls:
            out["masks"] = km.masks
        for k, v in vars(tr).items():                            # every loss the trainer holds after this call
            if k.startswith("loss_") and torch.is_tensor(v):
                out["losses"]["%d %s %s" % (len(out["calls"]), method, k)] = float(v.detach())

    run_iteration(tr, hp, FINAL_IT, dreal, pairs(), on_call)
    tr.dis_opt.settle()
    torch.cuda.synchronize()
    opts = {"gen": tr.gen_opt, "dis": tr.dis_opt}
    mods = {}
    if tr.use_classifier_sr:
        opts["feat"] = tr.classif_opt_sr
        mods = {"a": tr.domain_classifier_sr_a, "b": tr.domain_classifier_sr_b}
    if tr.use_output_classifier_sr:
        opts["out"] = tr.output_classif_opt_sr
    out["flat_p"] = {k: o.flat_p.detach().cpu().clone() for k, o in opts.items()}
    out["buffers"] = {pre + "." + k: v.detach().cpu().clone() for pre, m in mods.items() for k, v in m.named_buffers()}
    torch.save(out, os.path.join(tmpdir, "final_rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("name", ["FeatureDA", "Output_DA"])
def test_two_rank_iteration_of_the_final_test_configurations(tmp_path, monkeypatch, name):
    """FeatureDA.yaml and Output_DA.yaml (tests/golden/golden_final_configs.json through tests/final_configs.reduced_hp: that
    file's crop, depth and cadence) with data_parallel 1 and batch 1 per rank: iteration 1 -- the one on which the classifier
    updates fall -- in scripts/train.py's order (examples/train_loop.run_iteration) on two ranks.  Every optimizer's flat_p
    and every batch-norm buffer is bitwise equal across the ranks, every logged loss is finite, and the real-image
    loss_classifier_sr_update / loss_output_classifier_sr_update, its mean over the ranks, is within 1e-5 relative of the
    fp64 oracle's on the joined batch (the classifiers as the update met them, both ranks' kinks concatenated)."""
    import math
    from oracle import munit_oracle as O
    from tests import final_configs as C
    from tests import outda_oracle as U
    from tests import semantic_oracle as S
    ckpt = str(tmp_path / "seg.pth")
    torch.save({k: v.cpu() for k, v in S.make_model(0).state_dict().items()}, ckpt)
    _spawn(_final_worker, tmp_path, monkeypatch, 0, name, ckpt)
    r0, r1 = [torch.load(tmp_path / ("final_rank%d.pt" % k), weights_only=True) for k in range(2)]
    feature = name == "FeatureDA"
    want = [c[0] for c in C.CADENCE[name][FINAL_IT]]
    assert r0["calls"] == r1["calls"] == want, (r0["calls"], want)
    assert sorted(r0["flat_p"]) == sorted(["dis", "gen", "feat" if feature else "out"])
    for k in r0["flat_p"]:
        assert torch.equal(r0["flat_p"][k], r1["flat_p"][k]), k
    assert (len(r0["buffers"]) > 0) == feature and sorted(r0["buffers"]) == sorted(r1["buffers"])
    for k in r0["buffers"]:
        assert torch.equal(r0["buffers"][k], r1["buffers"][k]), k
    for r in (r0, r1):
        assert len(r["losses"]) >= len(want) and all(math.isfinite(v) for v in r["losses"].values()), r["losses"]
    for k in r0["sd_a"]:                                         # both ranks entered the update with the same classifiers
        assert torch.equal(r0["sd_a"][k], r1["sd_a"][k]) and torch.equal(r0["sd_b"][k], r1["sd_b"][k]), k
    hp = _final_hp(name, ckpt, 2)
    if feature:
        key = "%d domain_classifier_sr_update loss_classifier_sr_update" % (1 + want.index("domain_classifier_sr_update"))
        pins = _joint_pins(r0["sink"], r1["sink"])
        c_a, c_b = torch.cat([r0["codes"][0], r1["codes"][0]]), torch.cat([r0["codes"][1], r1["codes"][1]])
        ref = float(D.sr_loss(_oracle_state(r0["sd_a"]), _oracle_state(r0["sd_b"]), c_a, c_b, False, False, pins))
        assert pins.done() and pins.worst <= 5e-5, pins.worst                  # tests/parity.KINK_NOISE
    else:
        key = "%d output_domain_classifier_sr_update loss_output_classifier_sr_update" \
            % (1 + want.index("output_domain_classifier_sr_update"))
        sd_a = {k: v.double().clone() for k, v in r0["sd_a"].items()}
        sd_b = {k: v.double().clone() for k, v in r0["sd_b"].items()}
        real, synth = C.inputs(hp)
        km = O.KinkMasks([torch.cat([u, v], 0) for u, v in zip(r0["masks"], r1["masks"])], [])
        with pinned(km, name):
            ref = float(U.classifier_update(sd_a, sd_b, U.ClassifierOptimizer(sd_a, sd_b, hp), real[0].double(),
                                            synth[0].double(), real[1].double(), synth[1].double(), hp)[0])
    got = 0.5 * (r0["losses"][key] + r1["losses"][key])
    rel = abs(got - ref) / abs(ref)
    print("two-rank %s iteration %d: %s, %d losses finite, %s %.6f (mean over the ranks) oracle %.6f rel %.2e"
          % (name, FINAL_IT, want, len(r0["losses"]), key.split()[-1], got, ref, rel))
    assert rel <= 1e-5
