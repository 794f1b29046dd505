"""Host-side checks of the data-parallel adaptation terms (adaptation.data_parallel): the key's default, the refusals it lifts
and the ones it leaves, the C ABI of the cross-rank batch norm, and the sequence of collectives the two classifier updates
issue -- with torch.distributed recorded and every kernel replaced by a host stand-in, so no device is needed."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import munit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("munit_batchnorm_dp_workspace_bytes", "munit_batchnorm_dp_stats_local", "munit_batchnorm_dp_fwd_apply",
       "munit_batchnorm_dp_bwd_local", "munit_batchnorm_dp_bwd_finish")
FEAT = dict(adv_lambda=6, dfeat_lambda=1)
OUT = dict(output_classifier_lambda=1, output_adv_lambda=1)
OUT_KEYS = "output_adv_lambda.*output_classifier_lambda"


def _hp(size, **adaptation):
    hp = O.default_hp(size, 2, 1)
    hp["gen"]["n_res"] = 1
    hp["dis"]["num_scales"] = 1
    hp["adaptation"].update(adaptation)
    return hp


def test_the_key_defaults_to_0_and_lifts_only_the_data_parallel_refusals(monkeypatch):
    from munit_amd import trainer as T
    from munit_amd.utils import normalize_config
    assert normalize_config({})["adaptation"]["data_parallel"] == 0
    assert normalize_config({"adaptation": {"data_parallel": 1}})["adaptation"]["data_parallel"] == 1
    monkeypatch.setattr(T, "dp_size", lambda: 2)
    for key in ({}, {"data_parallel": 0}):                     # absent or 0: today's refusals
        with pytest.raises(NotImplementedError, match="adv_lambda.*dfeat_lambda.*data-parallel"):
            T.MUNIT_Trainer(_hp(256, **FEAT, **key))
        with pytest.raises(NotImplementedError, match=OUT_KEYS + ".*data-parallel"):
            T.MUNIT_Trainer(_hp(64, **OUT, **key))
    x = torch.zeros(1, 3, 256, 256)
    tr = T.MUNIT_Trainer(_hp(256, **FEAT, data_parallel=1))    # 1: both trainers construct under a world of 2 ...
    assert tr.use_classifier_sr and T.MUNIT_Trainer._bn_world(tr.hyperparameters) == 2
    tr.gen_opt.flat_g.fill_(3.0)
    tr.classif_opt_sr.flat_g.fill_(3.0)
    with pytest.raises(NotImplementedError, match="adv_lambda.*data-parallel"):      # ... and a step's hp without it is refused
        tr.gen_update(x, x, _hp(256, **FEAT))
    assert bool((tr.gen_opt.flat_g == 3.0).all()) and bool((tr.classif_opt_sr.flat_g == 3.0).all())
    tr = T.MUNIT_Trainer(_hp(64, **OUT, data_parallel=1))
    assert tr.use_output_classifier_sr
    monkeypatch.setattr(T, "dp_size", lambda: 1)               # one rank: the process's own statistics
    assert T.MUNIT_Trainer._bn_world(_hp(256, **FEAT, data_parallel=1)) == 0


def test_the_other_refusals_stay_with_the_key_at_1(monkeypatch):
    from munit_amd import trainer as T
    monkeypatch.setattr(T, "dp_size", lambda: 2)
    for prec in ("bf16", "bf16s"):
        hp = _hp(256, **FEAT, data_parallel=1)
        hp["precision"] = prec
        with pytest.raises(NotImplementedError, match="dfeat_lambda.*fp32 only"):
            T.MUNIT_Trainer(hp)
        hp = _hp(64, **OUT, data_parallel=1)
        hp["precision"] = prec
        with pytest.raises(NotImplementedError, match=OUT_KEYS + ".*fp32 only"):
            T.MUNIT_Trainer(hp)
    hp = _hp(64, **OUT, data_parallel=1)
    hp["optimizer"] = "extraadam"
    with pytest.raises(NotImplementedError, match=OUT_KEYS + ".*extrapolation"):
        T.MUNIT_Trainer(hp)
    with pytest.raises(ValueError, match="dfeat_lambda.*16..31"):
        T.MUNIT_Trainer(_hp(128, **FEAT, data_parallel=1))
    with pytest.raises(ValueError, match="adv_lambda.*dfeat_lambda"):
        T.MUNIT_Trainer(_hp(256, adv_lambda=6, data_parallel=1))
    for k in ("output_classifier_lambda", "output_adv_lambda"):     # the both-weights rule
        with pytest.raises(NotImplementedError, match=k):
            T.MUNIT_Trainer(_hp(64, data_parallel=1, **{k: 1}))
    with pytest.raises(NotImplementedError, match="sem_seg_lambda"):
        T.MUNIT_Trainer(_hp(256, **FEAT, sem_seg_lambda=1, data_parallel=1))
    for k in ("domain_adv_w", "vgg_w"):
        hp = _hp(256, **FEAT, data_parallel=1)
        hp[k] = 1
        with pytest.raises(NotImplementedError, match=k):
            T.MUNIT_Trainer(hp)


def test_new_symbols_are_declared_listed_and_exported():
    from munit_amd import _lib
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    declared = set(re.findall(r"\b(munit_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # host-side argument checks run before any launch (no device needed): negative return + munit_last_error
    big = 1 << 20
    # the backward's partials are doubles: 64 partial rows of 2 * C, and 2 * C totals
    assert lib.munit_batchnorm_dp_workspace_bytes(64) == 64 * 2 * 64 * 8 + 2 * 64 * 8 and lib.munit_batchnorm_dp_workspace_bytes(0) == 0
    assert lib.munit_batchnorm_dp_stats_local(8, 7, 64, 0, 0, 8, big, 8, big, None) == -1 and b"W = 0" in lib.munit_last_error()
    assert lib.munit_batchnorm_dp_stats_local(8, 7, 64, 65, 0, 8, big, 8, big, None) == -1
    assert lib.munit_batchnorm_dp_stats_local(8, 7, 64, 2, 2, 8, big, 8, big, None) == -1 and b"rank 2" in lib.munit_last_error()
    assert lib.munit_batchnorm_dp_stats_local(8, 1, 64, 1, 0, 8, big, 8, big, None) == -1      # N = 1
    assert b"more than one value" in lib.munit_last_error()
    assert lib.munit_batchnorm_dp_stats_local(8, 7, 6, 2, 0, 8, big, 8, big, None) == -1
    assert lib.munit_batchnorm_dp_stats_local(None, 7, 64, 2, 0, 8, big, 8, big, None) == -1
    assert lib.munit_batchnorm_dp_stats_local(8, 7, 64, 2, 0, 8, 2 * 3 * 64 - 1, 8, big, None) == -1
    assert b"exchange buffer" in lib.munit_last_error()
    assert lib.munit_batchnorm_dp_stats_local(8, 7, 64, 2, 0, 8, big, 8, 16, None) == -2
    assert lib.munit_batchnorm_dp_fwd_apply(8, 8, 8, 8, 8, 8, 7, 64, 2, 8, 2 * 3 * 64 - 1, 8, 8, 0, 1e-5, 0.1, None) == -1
    assert lib.munit_batchnorm_dp_fwd_apply(8, 8, None, 8, 8, 8, 7, 64, 2, 8, big, 8, 8, 0, 1e-5, 0.1, None) == -1
    assert lib.munit_batchnorm_dp_bwd_local(8, 8, None, 8, 8, 7, 64, 1, 2, 0, 8, big, 8, big, None) == -1      # ReLU without y
    assert lib.munit_batchnorm_dp_bwd_local(8, 8, 8, 8, 8, 7, 64, 1, 2, 0, 8, 2 * 4 * 64 - 1, 8, big, None) == -1
    assert lib.munit_batchnorm_dp_bwd_finish(8, 8, 8, 8, 8, 8, 8, None, None, 0.5, 7, 64, 1, 2, 0, 8, big, 8, big, None) == -1
    assert b"acc" in lib.munit_last_error()
    assert lib.munit_batchnorm_dp_bwd_finish(8, 8, 8, 8, 8, 8, 8, None, None, 0.0, 7, 64, 1, 2, 0, 8, big, 8, 16, None) == -2


# ---- the collectives of the two classifier updates ---------------------------------------------------------------------------
class _Group(object):
    """torch.distributed as one rank of a world of 2 sees it, every all_reduce recorded by size."""

    def __init__(self, monkeypatch, rank, log):
        import torch.distributed as dist
        monkeypatch.setattr(dist, "is_available", lambda: True)
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
        monkeypatch.setattr(dist, "get_rank", lambda *a: rank)
        monkeypatch.setattr(dist, "all_reduce", lambda t, *a, **k: log.append(("all_reduce", t.numel())))


def _host_ops(monkeypatch, log):
    """Every kernel the classifier updates reach, replaced: torch on the host for the plain layers, recorded no-ops for the
    cross-rank batch norm's entry points and the optimizer step."""
    from munit_amd import _lib, ops
    monkeypatch.setattr(ops, "_require", lambda *a, **k: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "workspace", lambda n, dev, stream=None: torch.empty(n, dtype=torch.uint8))
    monkeypatch.setattr(ops, "conv2d", lambda x, w, b=None, stride=1, pad=0, *a, **k: F.conv2d(x, w, b, stride, pad))
    monkeypatch.setattr(ops, "linear", lambda x, w, b=None, act="none": F.linear(x, w, b))
    monkeypatch.setattr(ops, "maxpool2", lambda x: F.max_pool2d(x, 2))
    monkeypatch.setattr(ops, "avgpool16", lambda x: F.avg_pool2d(x, (16, 16)).flatten(1))
    monkeypatch.setattr(ops, "add_relu", lambda a, r, link=None, dann=False: F.relu(a + r))
    monkeypatch.setattr(ops, "mse_const", lambda x, t: torch.mean((x - t) ** 2))
    monkeypatch.setattr(ops, "scalar_sum", lambda terms: sum(terms))
    monkeypatch.setattr(ops, "adam_step", lambda *a: log.append(("adam_step", a[0].numel())))
    lib = _lib.load()
    for name in NEW[1:]:
        monkeypatch.setattr(lib, name, (lambda n: lambda *a: log.append((n,)) or 0)(name))


def test_both_ranks_issue_the_same_collectives_in_a_feature_classifier_update(monkeypatch):
    """One domain_classifier_sr_update per rank of a world of 2: the forward's twelve statistics exchanges in program order
    (classifier a, then b; per classifier bn1, bn2 and the shortcut's norm of the 128- and of the 64-channel block, W * 3 * C
    floats each), the backward's twelve (W * 4 * C: two sums, each as two floats), then the flat gradient of classif_opt_sr -- and only then the optimizer
    step.  The same sequence on both ranks."""
    from munit_amd import trainer as T
    seqs = []
    for rank in (0, 1):
        log = []
        _Group(monkeypatch, rank, log)
        _host_ops(monkeypatch, log)
        torch.manual_seed(0)
        tr = T.MUNIT_Trainer(_hp(256, **FEAT, data_parallel=1))
        code = torch.randn(1, 256, 64, 64, generator=torch.Generator().manual_seed(7 + rank))
        tr._content_enc = lambda k: (lambda x: code)
        x = torch.zeros(1, 3, 256, 256)
        tr.domain_classifier_sr_update(x, x, False, 1.0, 0)
        seqs.append(log)
        monkeypatch.undo()
    assert seqs[0] == seqs[1]
    coll = [n for what, *rest in seqs[0] if what == "all_reduce" for n in rest]
    fwd = [2 * 3 * c for c in (128, 128, 128, 64, 64, 64)] * 2
    assert coll[:12] == fwd
    assert sorted(coll[12:24]) == sorted(2 * 4 * c for c in (128, 128, 128, 64, 64, 64) * 2)
    assert coll[24:] == [tr.classif_opt_sr.flat_g.numel()]
    names = [e[0] for e in seqs[0]]
    assert names[-2:] == ["all_reduce", "adam_step"]            # the exchange, then the step
    for i, e in enumerate(seqs[0][:-2]):                        # every exchange sits between its local and its finishing half
        if e[0] == "all_reduce":
            assert (names[i - 1], names[i + 1]) in (("munit_batchnorm_dp_stats_local", "munit_batchnorm_dp_fwd_apply"),
                                                    ("munit_batchnorm_dp_bwd_local", "munit_batchnorm_dp_bwd_finish")), i
    assert names.count("munit_batchnorm_dp_stats_local") == names.count("munit_batchnorm_dp_bwd_finish") == 12


def test_both_ranks_issue_the_same_collectives_in_an_output_classifier_update(monkeypatch):
    """output_domain_classifier_sr_update: MsImageDis has no batch statistics, so the one collective is the flat gradient of
    output_classif_opt_sr, between backward and step()."""
    from munit_amd import trainer as T
    seqs = []
    for rank in (0, 1):
        log = []
        _Group(monkeypatch, rank, log)
        _host_ops(monkeypatch, log)
        torch.manual_seed(0)
        hp = _hp(64, **OUT, data_parallel=1)
        tr = T.MUNIT_Trainer(hp)
        for cls in (tr.output_classifier_sr_a, tr.output_classifier_sr_b):        # the passes themselves are not under test
            cls.__dict__["calc_dis_loss_sr"] = (lambda c: lambda sim, real: sum((p * p).sum() for p in c.parameters()))(cls)
        x = torch.zeros(1, 3, 64, 64)
        tr.output_domain_classifier_sr_update(x, x, x, x, hp, 0)
        assert float(tr.output_classif_opt_sr.flat_g.abs().max()) > 0              # the backward reached the flat buffer
        seqs.append(log)
        monkeypatch.undo()
    assert seqs[0] == seqs[1] == [("all_reduce", tr.output_classif_opt_sr.flat_g.numel()),
                                  ("adam_step", tr.output_classif_opt_sr.flat_p.numel())]
