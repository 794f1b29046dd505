"""CPU (no GPU): the C-ABI library loads and exports every declared symbol, the host-side
mirror of the reference interface (module tree, state_dict keys, init RNG stream, config
defaults, LR schedule, optimizer state format) and the data-parallel exchange over gloo."""
import ctypes
import fnmatch
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import munit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_library_exports_every_declared_symbol(built):
    from munit_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "munit_hip.h")).read()
    declared = set(re.findall(r"\b(munit_[a-z0-9_]+)\s*\(", header))
    declared -= {"munit_stream_t"}
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.munit_version() >= 1


def test_host_arg_checks_without_gpu(built):
    """Argument validation happens on the host before any launch."""
    from ctypes import byref, c_int
    from munit_amd import _lib
    lib = _lib.load()
    d = _lib.ConvDesc(1, 4, 4, 8, 8, 3, 3, 1, 4, 1, 0, 0, 0.0)  # reflect pad 4 >= H
    ho, wo = c_int(), c_int()
    assert lib.munit_conv2d_out_hw(byref(d), byref(ho), byref(wo)) != 0
    assert b"reflect" in lib.munit_last_error()
    d = _lib.ConvDesc(2, 16, 16, 64, 128, 4, 4, 2, 1, 1, 0, 0, 0.0)
    assert lib.munit_conv2d_out_hw(byref(d), byref(ho), byref(wo)) == 0 and (ho.value, wo.value) == (8, 8)
    d = _lib.ConvDesc(2, 16, 16, 256, 128, 5, 5, 1, 2, 1, 1, 0, 0.0)
    assert lib.munit_conv2d_out_hw(byref(d), byref(ho), byref(wo)) == 0 and (ho.value, wo.value) == (32, 32)
    assert lib.munit_conv2d_dgrad_workspace_bytes(byref(d)) > 0
    assert lib.munit_conv2d_wgrad_workspace_bytes(byref(d)) > 0


def test_ops_refuse_cpu_tensors():
    from munit_amd import ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.instance_norm(torch.zeros(1, 4, 4, 4))


@pytest.mark.parametrize("gs", [1, 0])
def test_state_dict_layout_and_init_stream_match_reference(golden, gs):
    """Same seed -> same module tree, key order and initial weights as the reference's
    construction sequence (trainer.py:67-127 driven over the reference modules in
    make_golden.py)."""
    from munit_amd.trainer import MUNIT_Trainer
    meta, _ = golden
    g = meta["init_gs%d" % gs]
    hp = O.default_hp(64, 1, gs)
    torch.manual_seed(1234)
    tr = MUNIT_Trainer(hp)
    assert [k for k, _ in tr.named_parameters()] == g["keys"]
    assert list(tr.state_dict().keys()) == g["state_keys"]

    def dg(t):
        f = t.detach().double().reshape(-1)
        idx = torch.linspace(0, f.numel() - 1, 8).long()
        return [float(f.sum()), float(f.abs().sum()), float(f.norm())] + [float(v) for v in f[idx]]

    for (k, p), d in zip(tr.named_parameters(), g["digests"]):
        got = dg(p)
        assert max(abs(a - b) for a, b in zip(got, d)) <= 1e-6 * max(1.0, abs(d[1])), k
    assert max(abs(a - b) for a, b in zip(dg(tr.s_a), g["s_a"])) < 1e-6
    assert max(abs(a - b) for a, b in zip(dg(tr.s_b), g["s_b"])) < 1e-6


def test_param_counts_and_flat_buffers():
    from munit_amd.trainer import MUNIT_Trainer
    tr = MUNIT_Trainer(O.default_hp(64, 1, 1))
    assert sum(p.numel() for p in tr.gen.parameters()) == 27293590
    assert sum(p.numel() for p in tr.dis_a.parameters()) == 8271171
    # every parameter is a view into the optimizer's flat buffer, conv weights stored [O][KH][KW][I]
    w = tr.gen.enc_style.model[1].conv.weight
    assert w.shape == (128, 64, 4, 4) and w.stride() == (1024, 1, 256, 64)
    lo, hi = tr.gen_opt.flat_p.data_ptr(), tr.gen_opt.flat_p.data_ptr() + 4 * tr.gen_opt.flat_p.numel()
    for p in tr.gen.parameters():
        assert lo <= p.data_ptr() < hi and p.data_ptr() % 16 == 0
        assert p._munit_grad.shape == p.shape and p.grad is p._munit_grad
    tr2 = MUNIT_Trainer(O.default_hp(64, 1, 0))
    assert sum(p.numel() for p in tr2.gen_a.parameters()) == 15030291


def test_config_defaults_and_unsupported_losses(tmp_path):
    from munit_amd import get_config
    from munit_amd.trainer import MUNIT_Trainer
    import yaml
    hp = O.default_hp(64, 1, 1)
    del hp["adaptation"], hp["optimizer"]          # a stale config like config_HD.yaml
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(hp))
    conf = get_config(str(p))
    assert conf["optimizer"] == "adam" and conf["adaptation"]["adv_lambda"] == 0
    MUNIT_Trainer(conf)
    bad = O.default_hp(64, 1, 1)
    bad["semantic_w"] = 3
    with pytest.raises(NotImplementedError, match="semantic_w"):
        MUNIT_Trainer(bad)
    xa = O.default_hp(64, 1, 1)
    xa["optimizer"] = "extraadam"
    tr = MUNIT_Trainer(xa)
    assert type(tr.gen_opt).__name__ == "FusedExtraAdam"
    tr.iterations = 1
    with pytest.raises(RuntimeError, match="extrapolation"):
        tr.gen_opt_step()                           # step before any extrapolation, as in the reference


def test_lr_schedule_matches_reference_order():
    """scheduler stepped at the start of each iteration (train.py:172); StepLR(step_size, gamma)."""
    from munit_amd.trainer import MUNIT_Trainer
    hp = O.default_hp(64, 1, 1)
    hp["step_size"] = 2
    tr = MUNIT_Trainer(hp)
    lrs = []
    for _ in range(5):
        tr.update_learning_rate()
        lrs.append(tr.gen_opt.param_groups[0]["lr"])
    assert lrs == [O.step_lr(hp["lr"], n, hp) for n in range(1, 6)]
    assert tr.dis_opt.param_groups[0]["lr"] == lrs[-1]


def test_optimizer_state_dict_is_torch_adam_format():
    from munit_amd.trainer import MUNIT_Trainer
    tr = MUNIT_Trainer(O.default_hp(64, 1, 1))
    ref = torch.optim.Adam([torch.nn.Parameter(p.detach().clone(memory_format=torch.contiguous_format))
                            for p in tr.dis_opt._plist], lr=1e-4, betas=(0.5, 0.999), weight_decay=1e-4)
    for p in ref.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    ref.step()
    mine = tr.dis_opt
    mine.load_state_dict(ref.state_dict())
    assert mine._step == 1
    sd = mine.state_dict()
    assert set(sd) == {"state", "param_groups"} and len(sd["state"]) == len(mine._plist)
    for i, st in ref.state_dict()["state"].items():
        assert torch.equal(sd["state"][i]["exp_avg"], st["exp_avg"])
        assert sd["state"][i]["exp_avg"].is_contiguous()
    ref.load_state_dict(sd)  # and back


def test_checkpoint_names_and_key_layout(tmp_path):
    from munit_amd.trainer import MUNIT_Trainer
    hp = O.default_hp(64, 1, 1)
    tr = MUNIT_Trainer(hp)
    tr.save(str(tmp_path), 41)
    assert sorted(os.listdir(tmp_path)) == ["dis_00000042.pt", "gen_00000042.pt", "optimizer.pt"]
    sd = torch.load(tmp_path / "gen_00000042.pt", weights_only=True)
    assert list(sd) == ["2"] and sd["2"]["enc_style.model.0.conv.weight"].is_contiguous()
    tr2 = MUNIT_Trainer(hp)
    assert tr2.resume(str(tmp_path), hp) == 42
    for a, b in zip(tr.parameters(), tr2.parameters()):
        assert torch.equal(a, b)


def ckpt_ref_hp():
    """Hyper-parameters of the small geometry tests/golden/ckpt_ref was written for (make_golden_variants.py)."""
    import json
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_ref")
    exp = json.load(open(os.path.join(here, "expect.json")))
    hp = O.default_hp(32, 2, 1)
    hp["gen"], hp["dis"] = dict(exp["gen_cfg"]), dict(exp["dis_cfg"])
    return here, exp, hp


def test_resume_loads_a_checkpoint_written_by_the_reference_modules():
    """tests/golden/ckpt_ref holds gen_/dis_/optimizer.pt files produced by the REFERENCE's
    AdaINGen_double / MsImageDis `state_dict()` and torch.optim.Adam `state_dict()` in the reference's save format
    (scripts/trainer.py:1387-1429).  MUNIT_Trainer.resume must take them as they are (weights-only loader): key layout,
    iteration count from the file name, parameter values, Adam moments and step counter."""
    from munit_amd.trainer import MUNIT_Trainer
    from tests.test_oracle_golden import close_digest, dg
    here, exp, hp = ckpt_ref_hp()
    tr = MUNIT_Trainer(hp)
    assert list(tr.gen.state_dict().keys()) == exp["gen_keys"]
    assert list(tr.dis_a.state_dict().keys()) == exp["dis_keys"]
    assert tr.resume(here, hp) == exp["iterations"]
    for p, d in zip(tr.gen.parameters(), exp["gen_params"]):
        close_digest(dg(p), d, 1e-7)
    assert tr.gen_opt._step == int(exp["gen_opt_step"]) == 2 and tr.dis_opt._step == 2
    m0, _ = tr.gen_opt._views[0]
    _, v_last = tr.gen_opt._views[-1]
    close_digest(dg(m0), exp["gen_exp_avg0"], 1e-7)
    close_digest(dg(v_last), exp["gen_exp_avg_sq_last"], 1e-7)
    # and the files this build writes back carry the same keys and values (the reverse direction of the wire format)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        tr.save(d, 2)
        mine = torch.load(os.path.join(d, "gen_00000003.pt"), weights_only=True)["2"]
        theirs = torch.load(os.path.join(here, "gen_00000003.pt"), weights_only=True)["2"]
        assert list(mine) == list(theirs)
        for k in mine:
            assert mine[k].shape == theirs[k].shape and torch.equal(mine[k], theirs[k]), k
        o_mine = torch.load(os.path.join(d, "optimizer.pt"), weights_only=True)
        o_theirs = torch.load(os.path.join(here, "optimizer.pt"), weights_only=True)
        for which in ("gen", "dis"):
            assert set(o_mine[which]["state"]) == set(o_theirs[which]["state"])
            for i, st in o_theirs[which]["state"].items():
                assert torch.equal(o_mine[which]["state"][i]["exp_avg_sq"], st["exp_avg_sq"]), (which, i)
                assert float(o_mine[which]["state"][i]["step"]) == float(st["step"])


_DP_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %(root)r)
from munit_amd.trainer import MUNIT_Trainer
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=2)
r = dist.get_rank()
flat = torch.arange(10, dtype=torch.float32) * (r + 1)
MUNIT_Trainer._all_reduce_mean(flat)
assert torch.allclose(flat, torch.arange(10, dtype=torch.float32) * 1.5), flat
# bench.py's shard rule: rank r takes samples [r*B, (r+1)*B) of the global batch
import bench
xa, xb, ma, mb = bench.make_batch(2, 16, rank=r)
ga, _, _, _ = bench.make_batch(2, 16, rank=0), None, None, None
assert xa.shape == (2, 3, 16, 16)
g = [torch.zeros_like(xa) for _ in range(2)]
dist.all_gather(g, xa)
assert not torch.equal(g[0], g[1])          # ranks see different data
dist.barrier()
dist.destroy_process_group()
print("ok", r)
"""


def test_data_parallel_exchange_gloo_world2(tmp_path):
    """N > 1 path on CPU: mean all-reduce of the flat gradient + per-rank data shards."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "w.py"
    script.write_text(_DP_WORKER % dict(root=ROOT, port=port))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              cwd=ROOT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o


_XCH_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %(root)r)
from munit_amd import trainer as T
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=2)
r = dist.get_rank()
n = 1000
g = torch.Generator().manual_seed(50 + r)
grad = torch.randn(n, generator=g)                       # this rank's "flat gradient"
early = [(300, 520), (700, 1000)]                        # two ranges, as gen_state 0 has (decoder + MLP of gen_a and of gen_b)
# serial form: one all-reduce of the whole buffer
serial = grad.clone()
T.MUNIT_Trainer._all_reduce_mean(serial)
# overlapped form: stage 1 (the early ranges) goes out from a tensor hook in the middle of a backward pass, stage 2 (the "residual
# trunk" of the encoder) from a hook further down, the rest afterwards
flat = grad.clone()
enc_w = torch.ones(4, requires_grad=True)
trunk_w = torch.ones(4, requires_grad=True)
dec_w = torch.ones(4, requires_grad=True)
h = enc_w * 2.0                                           # "tensor entering the trunk": its gradient is formed after the trunk's
c = h * trunk_w                                           # "content code": its gradient is formed after the decoder's
fired_at = []
trunk = [(100, 260)]
xch = T.GradExchange(flat, T.dp_world()).arm(early, [c]).arm(trunk, [h])
trunk_w.register_hook(lambda g_: fired_at.append(("trunk", [st["fired"] for st in xch.stages])))
enc_w.register_hook(lambda g_: fired_at.append(("enc", [st["fired"] for st in xch.stages])))
loss = (dec_w * c).sum()
loss.backward()
# stage 1 was launched BEFORE the trunk's gradient existed, stage 2 BEFORE the encoder's first layer's
assert fired_at == [("trunk", [True, False]), ("enc", [True, True])], fired_at
assert xch.rest == [(0, 100), (260, 300), (520, 700)], xch.rest
xch.finish()
assert torch.equal(flat, serial), (flat - serial).abs().max()
# a stage whose tensors need no gradient is dropped: its ranges are exchanged in finish()
flat2 = grad.clone()
x2 = T.GradExchange(flat2, T.dp_world()).arm(early, [torch.ones(3)])
assert not x2.stages and not x2.fired and x2.rest == [(0, n)]
x2.finish()
assert torch.equal(flat2, serial)
# overlapping stages are a programming error
try:
    T.GradExchange(grad.clone(), T.dp_world()).arm(early, [c]).arm([(500, 600)], [c])
    raise SystemExit("overlap accepted")
except AssertionError:
    pass
other = [torch.zeros(n) for _ in range(2)]
dist.all_gather(other, grad)
assert torch.allclose(serial, (other[0] + other[1]) / 2)
dist.barrier()
dist.destroy_process_group()
print("ok", r)
"""


def test_overlapped_gradient_exchange_equals_the_serial_all_reduce_gloo_world2(tmp_path):
    """GradExchange (the decoder / MLP part of the flat generator gradient all-reduced from a hook inside backward, the
    rest after it) against the single all-reduce, two gloo ranks: bitwise equal, issued before the encoder gradient is formed."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "xch.py"
    script.write_text(_XCH_WORKER % dict(root=ROOT, port=port))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "ok" in o


def test_early_exchange_ranges_cover_decoders_and_mlps():
    """The flat-buffer ranges handed to GradExchange are exactly the decoder and MLP parameters (gen_state 1: one contiguous
    tail of the buffer; gen_state 0: one range per generator), 16-byte aligned; stage 2's are exactly the residual trunks of the
    two content encoders (one range each), disjoint from stage 1's."""
    from munit_amd.trainer import MUNIT_Trainer
    for gs, n_ranges in ((1, 1), (0, 2)):
        tr = MUNIT_Trainer(O.default_hp(64, 1, gs))
        r = tr._early_ranges
        assert len(r) == n_ranges and all(a % 4 == 0 and b % 4 == 0 for a, b in r), r
        gens = [("", tr.gen)] if gs == 1 else [("a.", tr.gen_a), ("b.", tr.gen_b)]
        names = [pre + n for pre, g in gens for n, _ in g.named_parameters()]
        offs = tr.gen_opt._offsets
        for n, p, off in zip(names, tr.gen_opt._plist, offs):
            late = ".dec" in "." + n or ".mlp" in "." + n
            inside = any(a <= off and off + p.numel() <= b for a, b in r)
            assert inside == late, (n, off, r)
        if gs == 1:
            assert r[0][1] == tr.gen_opt._total
        t = tr._trunk_ranges
        assert len(t) == 2 and all(a % 4 == 0 and b % 4 == 0 for a, b in t), t
        for n, p, off in zip(names, tr.gen_opt._plist, offs):
            in_trunk = ("content.model.3." in n)          # config_256.yaml: two down-samplings -> the ResBlocks are model.3
            inside = any(a <= off and off + p.numel() <= b for a, b in t)
            assert inside == in_trunk, (n, off, t)
        assert all(b <= c or d <= a for a, b in t for c, d in r)
        # 4 blocks x 2 convs x (256 * 256 * 9 + 256) parameters per encoder
        assert all(b - a == 8 * (256 * 256 * 9 + 256) for a, b in t), t


def test_bench_self_launches_ranks_from_a_bare_shell():
    """`python bench.py --gpus 2` without a launcher must start the two ranks itself (children of a GPU-free parent),
    relay rank 0's single JSON line and return 0; --dry-run keeps it on the CPU (gloo rendezvous + all-reduce)."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["parallelism"] == "dp2"
    # a launcher / --gpus mismatch is refused instead of silently running another world size
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, cwd=ROOT, env=env2, timeout=600)
    assert p.returncode != 0 and b"does not match" in p.stderr


def test_compute_mode_plumbing_without_gpu():
    """munit_conv_desc.compute / ops.set_compute: names, values and validation (no kernel is launched)."""
    import ctypes
    from munit_amd import _lib, ops
    assert _lib.COMPUTE == {"f32": 0, "bf16": 1, "f32x3": 2}
    fields = [f[0] for f in _lib.ConvDesc._fields_]
    assert fields[-4:] == ["slope", "compute", "in_dtype", "out_dtype"] and ctypes.sizeof(_lib.ConvDesc) == 16 * 4
    assert ops.get_compute() == "f32"
    ops.set_compute("f32x3")
    assert ops.get_compute() == "f32x3"
    ops.set_compute("f32")
    with pytest.raises(ValueError):
        ops.set_compute("fp16")
    lib = _lib.load()
    d = _lib.ConvDesc(1, 8, 8, 32, 32, 3, 3, 1, 1, 1, 0, 0, 0.0, 7, 0, 0)  # unknown compute mode
    ho, wo = ctypes.c_int(), ctypes.c_int()
    assert lib.munit_conv2d_out_hw(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) != 0
    assert b"compute" in lib.munit_last_error()
    # bf16 storage plumbing: "bf16s" multiplies like "bf16"; tensor dtypes travel in the descriptor and are validated
    ops.set_compute("bf16s")
    assert ops.get_compute() == "bf16"
    ops.set_compute("f32")
    d = _lib.ConvDesc(1, 8, 8, 32, 64, 3, 3, 1, 1, 1, 0, 0, 0.0, 1, 1, 1)  # bf16 input with 32 channels: refused
    assert lib.munit_conv2d_out_hw(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) != 0
    assert b"Cin % 64" in lib.munit_last_error()
    d = _lib.ConvDesc(2, 8, 8, 64, 128, 3, 3, 1, 1, 1, 0, 0, 0.0, 1, 1, 1)
    assert lib.munit_conv2d_out_hw(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) == 0
    # the forward of a bf16-input layer multiplies by a bf16 copy of the weights; backward-data by the bf16 transpose
    assert lib.munit_conv2d_prepared_weight_bytes(ctypes.byref(d), 0) == 128 * 9 * 64 * 2
    assert lib.munit_conv2d_prepared_weight_bytes(ctypes.byref(d), 1) == 128 * 9 * 64 * 2
    # fp32 3x3 / stride 1 / pad 1 with wide channels: both passes multiply by a Winograd image (16 frequencies per channel pair)
    d32 = _lib.ConvDesc(2, 8, 8, 64, 128, 3, 3, 1, 1, 1, 0, 0, 0.0, 0, 0, 0)
    assert lib.munit_conv2d_prepared_weight_bytes(ctypes.byref(d32), 0) == 16 * 64 * 128 * 4
    assert lib.munit_conv2d_prepared_weight_bytes(ctypes.byref(d32), 1) == 16 * 64 * 128 * 4
    for which, kind in ((0, 4), (1, 5)):      # MUNIT_PREP_WINOGRAD, MUNIT_PREP_WINOGRAD_DGRAD
        item = _lib.PrepItem()
        assert lib.munit_conv2d_prep_item(ctypes.byref(d32), which, None, None, ctypes.byref(item)) == 0 and item.kind == kind
    # odd extent: the direct kernels (forward: the weights as they are; backward-data: their transpose)
    dodd = _lib.ConvDesc(2, 9, 8, 64, 128, 3, 3, 1, 1, 1, 0, 0, 0.0, 0, 0, 0)
    assert lib.munit_conv2d_prepared_weight_bytes(ctypes.byref(dodd), 0) == 0
    assert lib.munit_conv2d_prepared_weight_bytes(ctypes.byref(dodd), 1) == 128 * 9 * 64 * 4
    # nearest-x2 + 5x5 reflect-pad-2: four merged 3x3 phase filters, as Winograd images when the source extent is even
    dup = _lib.ConvDesc(2, 8, 8, 128, 64, 5, 5, 1, 2, 1, 1, 0, 0.0, 0, 0, 0)
    item = _lib.PrepItem()
    assert lib.munit_conv2d_prep_item(ctypes.byref(dup), 0, None, None, ctypes.byref(item)) == 0 and item.kind == 6
    assert lib.munit_conv2d_prepared_weight_bytes(ctypes.byref(dup), 0) == 4 * 16 * 128 * 64 * 4


def test_winograd_algebra_of_the_kernels():
    """The identities conv_wino.hip is built on, in fp64 numpy: F(2x2,3x3) and F(3x3,2x2) forward, their backward-weight form
    dg = G^T [(A dY A^T) . (B^T d B)] G, the reflect fold of the 3x3 backward-data done inside the input patch, and the
    parity split of the 4x4 / stride 2 layer (forward over four input phases; backward-data as four 2-tap phase planes whose
    padded rows fold onto their neighbours)."""
    import numpy as np
    rng = np.random.default_rng(0)
    BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], float)
    G3 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], float)
    AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], float)
    G2 = np.array([[1, 0], [.5, .5], [.5, -.5], [0, 1]], float)
    AT3 = np.array([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, -1]], float)

    def corr(d, g, m):   # VALID correlation, m x m outputs
        r = g.shape[0]
        return np.array([[(d[i:i + r, j:j + r] * g).sum() for j in range(m)] for i in range(m)])

    d = rng.standard_normal((4, 4))
    for G, AT, r, m in ((G3, AT2, 3, 2), (G2, AT3, 2, 3)):
        g = rng.standard_normal((r, r))
        y = AT @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ AT.T
        assert np.abs(y - corr(d, g, m)).max() < 1e-13
        dy = rng.standard_normal((m, m))
        dg = G.T @ ((AT.T @ dy @ AT) * (BT @ d @ BT.T)) @ G
        ref = np.array([[(dy * d[a:a + m, b:b + m]).sum() for b in range(r)] for a in range(r)])
        assert np.abs(dg - ref).max() < 1e-13

    # 1-D reflect-pad-1 3-tap layer, H = 8: dx = P^T C^T dy.  Kernel form: zero-padded correlation of dy with the flipped
    # filter, 2-output tiles over patches dy[2t-1 .. 2t+2]; top tile: patch row 3 += patch row 1, bottom tile: row 0 += row 2.
    H, w = 8, rng.standard_normal(3)
    x = rng.standard_normal(H)
    dyv = rng.standard_normal(H)
    xp = np.concatenate([[x[1]], x, [x[H - 2]]])
    dxp = np.zeros(H + 2)
    for o in range(H):
        dxp[o:o + 3] += dyv[o] * w
    dx_ref = dxp[1:H + 1].copy(); dx_ref[1] += dxp[0]; dx_ref[H - 2] += dxp[H + 1]
    dyz = np.concatenate([[0.0], dyv, [0.0, 0.0]])
    dx = np.zeros(H)
    for t in range(H // 2):
        p = dyz[2 * t:2 * t + 4].copy()                      # dy rows 2t-1 .. 2t+2
        if t == 0: p[3] += p[1]
        if t == H // 2 - 1: p[0] += p[2]
        for i in range(2):
            dx[2 * t + i] = sum(p[i + s] * w[2 - s] for s in range(3))
    assert np.abs(dx - dx_ref).max() < 1e-13
    assert abs(float((xp[0:3] * w).sum()) - float(sum(xp[k] * w[k] for k in range(3)))) < 1e-13   # (orientation of w)

    # 1-D 4-tap / stride 2 / reflect-pad-1 layer, H = 8 -> 4 outputs: forward = sum over the input parities r of 2-tap
    # correlations over phase plane X_r[q] = xp[2q + r]; backward-data = parity planes dxp[2u + par] = sum_a dy[u-a] w[2a+par],
    # image row = padded row - 1, padded rows 0 and H+1 folding onto rows 1 and H-2
    w4 = rng.standard_normal(4)
    y = np.array([(xp[2 * o:2 * o + 4] * w4).sum() for o in range(H // 2)])
    yp = np.zeros(H // 2)
    for r in range(2):
        Xr = xp[r::2]                                        # H/2 + 1 rows
        yp += np.array([Xr[o] * w4[r] + Xr[o + 1] * w4[2 + r] for o in range(H // 2)])
    assert np.abs(y - yp).max() < 1e-13
    dyo = rng.standard_normal(H // 2)
    dxp = np.zeros(H + 2)
    for o in range(H // 2):
        dxp[2 * o:2 * o + 4] += dyo[o] * w4
    dx_ref = dxp[1:H + 1].copy(); dx_ref[1] += dxp[0]; dx_ref[H - 2] += dxp[H + 1]
    dx = np.zeros(H)
    Hd = H // 2
    for par in range(2):
        plane = np.array([sum((dyo[u - a] if 0 <= u - a < Hd else 0.0) * w4[2 * a + par] for a in range(2)) for u in range(Hd + 1)])
        if par == 0:
            plane[1] += plane[0]                             # padded row 0 -> image row 1 (same plane, u = 1)
        else:
            plane[Hd - 1] += plane[Hd]                       # padded row H+1 -> image row H-2 (same plane, u = Hd-1)
        for u in range(Hd + 1):
            i = 2 * u + par - 1
            if 0 <= i < H and not (par == 0 and u == 0) and not (par == 1 and u == Hd):
                dx[i] = plane[u]
    assert np.abs(dx - dx_ref).max() < 1e-13


def test_trainer_method_surface_is_the_reference_s():
    """The methods of MUNIT_Trainer a training / test script of the reference calls (scripts/trainer.py: __init__ 29, the
    optimizer steps 252-268, recon_criterion(_mask) 279-305, forward 307, gen_update 336-346, sample 773, sample_syn 930,
    sample_fid 1087, dis_update 1133, update_learning_rate 1326, resume 1337, save 1387), by name and by parameter list."""
    import inspect
    from munit_amd.trainer import MUNIT_Trainer
    want = {
        "__init__": ["self", "hyperparameters"],
        "dis_opt_step": ["self"], "gen_opt_step": ["self"],
        "recon_criterion": ["self", "input", "target"],
        "recon_criterion_mask": ["self", "input", "target", "mask"],
        "forward": ["self", "x_a", "x_b"],
        "gen_update": ["self", "x_a", "x_b", "hyperparameters", "mask_a", "mask_b", "comet_exp", "synth", "semantic_gt_a",
                       "semantic_gt_b"],
        "dis_update": ["self", "x_a", "x_b", "hyperparameters", "comet_exp"],
        "sample": ["self", "x_a", "x_b"], "sample_syn": ["self", "x_a", "x_b"], "sample_fid": ["self", "x_a", "x_b"],
        "update_learning_rate": ["self"],
        "resume": ["self", "checkpoint_dir", "hyperparameters"],
        "save": ["self", "snapshot_dir", "iterations"],
    }
    for name, params in want.items():
        fn = getattr(MUNIT_Trainer, name)
        assert list(inspect.signature(fn).parameters) == params, (name, list(inspect.signature(fn).parameters))
    sig = inspect.signature(MUNIT_Trainer.gen_update).parameters
    assert sig["comet_exp"].default is None and sig["synth"].default is False and sig["semantic_gt_a"].default is None


def test_data_parallel_host_hooks_without_a_device():
    """Host wiring of the data-parallel schedule on a CPU-built trainer (no kernel runs): the discriminators call the
    wait of their optimizer's gate at the top of forward() -- calc_gen_loss / calc_dis_loss reach forward() directly, as the reference's do
    (networks.py:84-85, 104), so a module pre-hook would miss them --, the wait and the settle are no-ops while nothing is
    pending, apply() on the trainer or on a sub-network works before any device buffer exists, the content encoders hand out the
    tensor that enters their residual trunk only when asked, and the optimizer-step deferral is not taken without a process group."""
    from munit_amd import trainer as T
    from munit_amd.utils import weights_init
    tr = T.MUNIT_Trainer(O.default_hp(64, 1, 1))
    for d in (tr.dis_a, tr.dis_b):
        assert d.before_forward == tr.dis_opt.gate.wait
    gate = tr.dis_opt.gate
    assert gate.pending is None and gate.wait() is None
    tr.dis_opt.settle()
    assert gate.pending is None and gate.waited == set() and tr.last_exchange is None
    w0 = tr.dis_a.cnns[0][0].conv.weight.detach().clone()
    torch.manual_seed(5)
    tr.dis_a.apply(weights_init("gaussian"))            # sub-network apply with the image refresh tail: no optimizer buffer on a device yet
    tr.apply(weights_init("kaiming"))
    assert not torch.equal(w0, tr.dis_a.cnns[0][0].conv.weight)
    enc = tr._content_enc(1)
    assert enc is tr.gen.enc1_content and tr._content_enc(2) is tr.gen.enc2_content
    assert enc.keep_trunk_in is False and enc.trunk_in is None
    assert T.dp_world() == 0                             # no process group: gen_update / dis_update take the in-line path
    assert T.OVERLAP_EXCHANGE
    # the state_dict of a discriminator goes through the wait as well (registered pre-hook) and is unchanged by it
    assert list(tr.dis_a.state_dict().keys())[:2] == ["cnns.0.0.conv.weight", "cnns.0.0.conv.bias"]


class _Event(object):
    """Stand-in for the event a deferred step records."""


class _Stream(object):
    """Stand-in for a device stream: a handle, and the events it was told to wait for."""

    def __init__(self, handle):
        self.cuda_stream, self.waits = handle, []

    def wait_event(self, ev):
        self.waits.append(ev)


def _streams(monkeypatch, *handles):
    """Stand-in streams; the first is current, `use(s)` makes another one current (where StepGate asks torch for it)."""
    sts = [_Stream(h) for h in handles]
    cur = [sts[0]]
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: cur[0])
    return sts, lambda s: cur.__setitem__(0, s)


def _reached(fn):
    """Every object a callable holds on to: through __self__, __func__, __closure__, a hook wrapper's `hook`, a partial's
    parts, and the attributes of a StepGate."""
    from munit_amd.trainer import StepGate
    seen, todo = {}, [fn]
    while todo:
        o = todo.pop()
        if o is None or id(o) in seen:
            continue
        seen[id(o)] = o
        todo += [getattr(o, a, None) for a in ("__self__", "__func__", "__wrapped__", "hook", "func")]
        todo += [c.cell_contents for c in (getattr(o, "__closure__", None) or ())]
        todo += list(getattr(o, "args", None) or ()) if hasattr(o, "func") else []
        if isinstance(o, StepGate):
            for v in vars(o).values():
                todo += list(v) if isinstance(v, (set, list, tuple)) else [v]
    return list(seen.values())


def test_a_copy_of_a_discriminator_takes_an_idle_gate_and_nothing_of_the_trainer():
    """copy.deepcopy of dis_a / dis_b (EMA, snapshot copies): the memo holds neither the trainer nor an optimizer, the copy's
    forward hook and its state_dict / load_state_dict hooks reach no MUNIT_Trainer and no FusedAdam, and they hold a gate of
    their own on which nothing is pending -- also when the original's gate is armed."""
    import copy
    from munit_amd import trainer as T
    tr = T.MUNIT_Trainer(O.default_hp(64, 1, 1))
    tr.dis_opt.gate.arm(_Event())
    for d in (tr.dis_a, tr.dis_b):
        memo = {}
        c = copy.deepcopy(d, memo)
        assert not {id(tr), id(tr.gen_opt), id(tr.dis_opt)} & set(memo)
        hooks = [c.before_forward] + list(c._state_dict_pre_hooks.values()) + list(c._load_state_dict_pre_hooks.values())
        assert len(hooks) == 3 and all(h is not None for h in hooks)
        gates = set()
        for h in hooks:
            objs = _reached(h)
            assert not [o for o in objs if isinstance(o, (T.MUNIT_Trainer, T.FusedAdam))], h
            gates |= {id(o) for o in objs if isinstance(o, T.StepGate)}
        gate = c.before_forward.__self__
        assert gates == {id(gate)} and isinstance(gate, T.StepGate) and gate is not tr.dis_opt.gate
        assert gate.pending is None and gate.event is None and gate.waited == set()
        for p in c.parameters():                       # the copy's parameters belong to no optimizer
            assert getattr(p, "_munit_opt", None) is None
    assert tr.dis_opt.gate.pending is not None          # the original is as it was
    # the hooks of the original hold the gate as well, nothing larger
    for h in [tr.dis_a.before_forward] + list(tr.dis_a._state_dict_pre_hooks.values()):
        assert not [o for o in _reached(h) if isinstance(o, (T.MUNIT_Trainer, T.FusedAdam))]


def test_step_gate_waits_once_per_stream_and_settles(monkeypatch):
    """StepGate on stand-in events and streams: arm, then one wait_event per stream however often it asks; settle waits on
    the current stream if it has not yet and leaves nothing pending and nobody recorded; an idle gate calls nothing."""
    import copy
    from munit_amd.trainer import StepGate
    (a, b, c), use = _streams(monkeypatch, 11, 22, 33)
    gate = StepGate()
    gate.wait()
    gate.settle()
    assert gate.pending is None and gate.waited == set() and not (a.waits or b.waits or c.waits)
    ev = _Event()
    gate.arm(ev)
    assert gate.pending is ev and gate.waited == set()
    gate.wait()
    assert a.waits == [ev] and gate.waited == {11}
    gate.wait()
    assert a.waits == [ev]                              # the second wait on the same stream calls nothing
    use(b)
    gate.wait()
    assert b.waits == [ev] and a.waits == [ev] and gate.waited == {11, 22}
    use(c)
    gate.settle()                                       # this stream has not waited yet: it does, then nothing pends
    assert c.waits == [ev] and gate.pending is None and gate.waited == set()
    gate.arm(ev)
    use(a)
    gate.wait()
    gate.settle()                                       # this one has: no second wait
    assert a.waits == [ev, ev] and gate.pending is None and gate.waited == set()
    gate.wait()
    gate.settle()
    assert a.waits == [ev, ev] and b.waits == [ev] and c.waits == [ev]
    # a copy is a fresh gate; re-binding the optimizer drops the event with the device it belonged to
    gate.arm(ev, "dev0")
    twin = copy.deepcopy(gate)
    assert twin is not gate and twin.pending is None and twin.event is None and twin.device is None and twin.waited == set()
    gate.reset()
    assert a.waits == [ev, ev, ev] and gate.pending is None and gate.event is None and gate.device is None


def test_every_host_side_entry_settles_the_optimizers_gate(monkeypatch):
    """With a step pending on dis_opt's gate (stand-in event), each host-side way to the discriminators' weights or the
    optimizer's buffers waits exactly once on the current stream and leaves the gate idle; the generator's optimizer has a
    gate of its own and does not wait for the discriminators'."""
    from munit_amd import ops, trainer as T
    from munit_amd.utils import weights_init
    tr = T.MUNIT_Trainer(O.default_hp(64, 1, 1))
    (st,), _ = _streams(monkeypatch, 7)
    gate = tr.dis_opt.gate
    assert tr.gen_opt.gate is not gate and isinstance(tr.gen_opt.gate, T.StepGate)
    osd = tr.dis_opt.state_dict()
    msd = {k: v.detach().clone() for k, v in tr.dis_a.state_dict().items()}
    entries = [
        ("dis_opt.state_dict", lambda: tr.dis_opt.state_dict()),
        ("dis_opt.load_state_dict", lambda: tr.dis_opt.load_state_dict(osd)),
        ("dis_opt.zero_grad", lambda: tr.dis_opt.zero_grad()),
        ("dis_opt.invalidate_prepared", lambda: tr.dis_opt.invalidate_prepared()),
        ("dis_opt.settle", lambda: tr.dis_opt.settle()),
        ("dis_a.state_dict", lambda: tr.dis_a.state_dict()),
        ("dis_a.load_state_dict", lambda: tr.dis_a.load_state_dict(msd)),
        ("dis_b.load_state_dict", lambda: tr.dis_b.load_state_dict(msd)),
        ("dis_a.apply", lambda: tr.dis_a.apply(weights_init("gaussian"))),
        ("trainer.apply", lambda: tr.apply(weights_init("kaiming"))),
        ("trainer.state_dict", lambda: tr.state_dict()),
        ("trainer.to", lambda: tr.to("cpu")),
        ("dis_opt.bind", lambda: tr.dis_opt.bind(torch.device("cpu"))),
    ]
    for name, entry in entries:
        ev = _Event()
        gate.arm(ev)
        del st.waits[:]
        entry()
        assert st.waits == [ev], (name, st.waits)
        assert gate.pending is None and gate.waited == set(), name
        entry()                                         # nothing pending: nothing waits
        assert st.waits == [ev], name
    # the step methods settle as well (the kernel itself is not under test)
    steps = []
    monkeypatch.setattr(ops, "adam_step", lambda *a: steps.append(a[0]))
    ev = _Event()
    gate.arm(ev)
    del st.waits[:]
    tr.gen_opt.step()
    assert steps == [tr.gen_opt.flat_p] and st.waits == [] and gate.pending is ev      # not the generator's business
    tr.dis_opt.step()
    assert steps[-1] is tr.dis_opt.flat_p and st.waits == [ev] and gate.pending is None


def test_step_on_orders_exchange_step_and_event_on_the_given_stream(monkeypatch):
    """FusedAdam.step_on on stand-ins: the stream is ordered behind the caller's, `before` and the step run under it, the
    event is recorded on it after them, and only then is the gate armed; the next entry waits for that event."""
    import contextlib
    from munit_amd import ops, trainer as T
    tr = T.MUNIT_Trainer(O.default_hp(64, 1, 1))
    (main, comm), _ = _streams(monkeypatch, 1, 2)
    comm.device = torch.device("cpu")
    log = []

    class Ev(_Event):
        def record(self, stream):
            log.append(("record", stream.cuda_stream))

    @contextlib.contextmanager
    def under(stream):
        log.append(("enter", stream.cuda_stream))
        yield
        log.append(("exit", stream.cuda_stream))

    monkeypatch.setattr(torch.cuda, "Event", Ev)
    monkeypatch.setattr(torch.cuda, "stream", under)
    monkeypatch.setattr(ops, "stream_wait", lambda s, on: log.append(("stream_wait", s.cuda_stream, on.cuda_stream)))
    monkeypatch.setattr(ops, "adam_step", lambda *a: log.append(("adam_step", tr.dis_opt.gate.pending)))
    opt = tr.dis_opt
    opt.step_on(comm, before=lambda: log.append(("before", opt.gate.pending)))
    assert log == [("stream_wait", 2, 1), ("enter", 2), ("before", None), ("adam_step", None), ("record", 2), ("exit", 2)], log
    ev = opt.gate.pending
    assert isinstance(ev, Ev) and opt.gate.event is ev and opt.gate.device == comm.device and opt._step == 1
    opt.zero_grad()
    assert main.waits == [ev] and opt.gate.pending is None
    # the step to run is the caller's choice (the trainer passes dis_opt_step: ExtraAdam extrapolates on even iterations)
    del log[:]
    opt.step_on(comm, step=lambda: log.append(("my step",)))
    assert [e[0] for e in log] == ["stream_wait", "enter", "my step", "record", "exit"] and opt.gate.pending is ev
    opt.bind(torch.device("cpu"))                       # re-binding settles and drops the event
    assert main.waits == [ev, ev] and opt.gate.pending is None and opt.gate.event is None


def test_the_three_mean_all_reduces_are_one_function(monkeypatch):
    """MUNIT_Trainer._all_reduce_mean, GradExchange.finish and the exchange of the deferred discriminator step all go
    through trainer.all_reduce_mean; the function itself issues the collectives in the order given, waits for the stages that
    went out earlier and scales once."""
    import torch.distributed as dist
    from munit_amd import trainer as T
    real = T.all_reduce_mean
    calls = []
    monkeypatch.setattr(T, "all_reduce_mean", lambda *a, **k: calls.append((a, k)))
    monkeypatch.setattr(T, "dp_world", lambda: 2)
    flat = torch.arange(12, dtype=torch.float32)
    T.MUNIT_Trainer._all_reduce_mean(flat)
    assert len(calls) == 1 and calls[0][0][0] is flat and calls[0][0][1] == 2
    xch = T.GradExchange(flat, 2)
    xch.stages.append({"ranges": [(4, 8)], "pending": 0, "fired": True})
    xch.works.append("work")
    xch.finish()
    assert len(calls) == 2
    a, k = calls[1]
    assert a[0] is flat and a[1] == 2 and list(a[2:]) + list(k.values()) == [[(0, 4), (8, 12)], ["work"]]
    tr = T.MUNIT_Trainer(O.default_hp(64, 1, 1))
    kept = {}
    monkeypatch.setattr(T, "comm_stream", lambda dev: "comm")
    monkeypatch.setattr(tr.dis_opt, "step_on", lambda stream, before=None, step=None: kept.update(stream=stream, before=before, step=step))
    tr._defer_dis_step(torch.device("cpu"))
    assert kept["stream"] == "comm" and kept["step"] == tr.dis_opt_step and len(calls) == 2
    kept["before"]()
    assert len(calls) == 3 and calls[2][0][0] is tr.dis_opt.flat_g and calls[2][0][1] == 2
    # the function: whole buffer / ranges in order, then the waits, then one scale; world 1 does not scale
    log = []
    monkeypatch.setattr(dist, "all_reduce", lambda t, *a, **k: log.append(("all_reduce", t.data_ptr(), t.numel())))

    class Work(object):
        def wait(self):
            log.append(("wait",))

    x = torch.full((12,), 3.0)
    real(x, 2)
    assert log == [("all_reduce", x.data_ptr(), 12)] and torch.equal(x, torch.full((12,), 1.5))
    del log[:]
    real(x, 2, [(0, 4), (8, 12)], [Work()])
    assert log == [("all_reduce", x.data_ptr(), 4), ("all_reduce", x[8:].data_ptr(), 4), ("wait",)]
    assert torch.equal(x, torch.full((12,), 0.75))
    real(x, 1)
    assert torch.equal(x, torch.full((12,), 0.75))



def test_bench_sizes_host_threads_from_the_granted_cpus(monkeypatch):
    """bench.py's thread pools (the ranks it launches, the CPU-baseline leg) are sized from the CPUs the process may use --
    affinity mask capped by the cgroup quota, the rule of tests/conftest.usable_cpus -- never from os.cpu_count(), which on
    the GPU boxes reports 256 for a grant of 16."""
    import bench
    from tests.conftest import usable_cpus
    assert bench.usable_cpus() == usable_cpus()
    monkeypatch.setattr(os, "cpu_count", lambda: 4096)         # what the box SHOWS must not matter
    n = bench.usable_cpus()
    assert n == usable_cpus() and n <= len(os.sched_getaffinity(0))
    assert bench.host_cores() <= n
    assert bench.rank_threads(1) == n and bench.rank_threads(8) == max(1, n // 8) and bench.rank_threads(10 * n) == 1
    monkeypatch.setattr(bench, "cpu_quota", lambda: 3)          # a quota below the affinity mask wins
    assert bench.usable_cpus() == min(3, len(os.sched_getaffinity(0)))
    assert bench.rank_threads(2) == max(1, bench.usable_cpus() // 2)
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert src.count("os.cpu_count()") == 2                     # the docstring and the no-sched_getaffinity fallback of usable_cpus


def test_kernel_names_reported_by_the_library_exist_in_the_committed_trace():
    """munit_conv2d_kernel_name feeds bench.py's roofline table and its lookup in the PMC summary: a name of a kernel that does
    not run (round 3: the image head's backward-weight was reported as conv_lanes_wgrad_kernel while conv_lanes_wgrad_pk_kernel
    ran) silently drops the traffic figure.  For the dominant layers of BASELINE configs[1] every reported kernel must appear in
    the newest committed rocprofv3 by-grid trace of that workload -- Winograd instantiations with their exact template
    arguments, the others by kernel name."""
    import glob
    import re
    from munit_amd import _lib, ops
    traces = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_kernel_trace_by_grid_single_stream_bench_256_b8.txt")))
    assert traces, "no committed kernel trace"
    text = open(traces[-1]).read()
    lib = _lib.load()
    lib.munit_conv2d_kernel_name.restype = ctypes.c_char_p
    layers = [(8, 64, 64, 256, 256, 3, 1, 1, False), (8, 256, 256, 64, 128, 4, 2, 1, False), (8, 128, 128, 128, 256, 4, 2, 1, False),
              (8, 64, 64, 256, 128, 5, 1, 2, True), (8, 128, 128, 128, 64, 5, 1, 2, True), (8, 256, 256, 64, 3, 7, 1, 3, False),
              (8, 256, 256, 3, 64, 7, 1, 3, False), (16, 128, 128, 64, 128, 4, 2, 1, False)]
    seen = set()
    for (b, h, w, ci, co, k, s, p, up) in layers:
        pl = ops._plan(b, h, w, ci, co, k, k, s, p, "reflect", up, "none", 0.2, 0, 0)
        for which in (0, 1, 2):
            name = lib.munit_conv2d_kernel_name(pl.ref, which).decode()
            for part in re.split(r" \+ | x4 ", name):
                part = part.split(" (")[0].strip()
                m = re.match(r"([a-z_0-9]+_kernel)(<[^>]*>)?", part)
                if not m:
                    continue
                base, targs = m.group(1), m.group(2)
                exact = base + targs if (targs and "." not in targs and base.startswith("conv_wino")) else base
                seen.add(exact)
                assert exact[:44] in text, (name, exact, os.path.basename(traces[-1]))
    assert "conv_lanes_wgrad_pk_kernel" in seen and "conv_wino_kernel<0, 0>" in seen and len(seen) >= 10, seen


# ---- the parity harness's own plumbing: ops.kinks, O.pinned, tests/parity.pinned ------------------------------------------
SINKS = ("MASK_SINK", "L1_SINK", "SEG_SINK", "DANN_SINK")


def _sinks():
    from munit_amd import ops
    return tuple(getattr(ops, s) for s in SINKS)


def test_kinks_records_into_fresh_and_passed_lists_and_restores():
    from munit_amd import ops
    assert _sinks() == (None,) * 4
    mine = ["held by the oracle side"]
    with ops.kinks(mask=True, seg=mine) as k:
        assert k.mask == [] and ops.MASK_SINK is k.mask                 # True: a fresh list, and the global is that list
        assert ops.SEG_SINK is mine and k.seg is mine                   # a passed list is used as is
        assert ops.L1_SINK is None and ops.DANN_SINK is None and k.l1 is None and k.dann is None    # not named: left alone
        ops.MASK_SINK.append(1)
        with ops.kinks(l1=True) as inner:                               # not named here: the outer lists stay active
            assert ops.MASK_SINK is k.mask and inner.mask is k.mask and inner.seg is mine and inner.l1 == []
        assert ops.L1_SINK is None
    assert _sinks() == (None,) * 4 and k.mask == [1] and mine == ["held by the oracle side"]


def test_kinks_none_switches_a_channel_off_inside_a_recording_block():
    from munit_amd import ops
    with ops.kinks(mask=True, l1=True) as k:
        ops.MASK_SINK.append("before")
        with ops.kinks(mask=None) as off:
            assert ops.MASK_SINK is None and off.mask is None
            assert ops.L1_SINK is k.l1 and off.l1 is k.l1
        assert ops.MASK_SINK is k.mask and k.mask == ["before"]         # the outer list is back, with its contents
    assert _sinks() == (None,) * 4


def test_kinks_restores_when_the_block_raises_and_refuses_unknown_names():
    from munit_amd import ops
    outer = []
    with ops.kinks(dann=outer):
        with pytest.raises(ZeroDivisionError):
            with ops.kinks(mask=True, l1=True, seg=True, dann=None):
                assert ops.DANN_SINK is None and ops.SEG_SINK == []
                1 / 0
        assert _sinks() == (None, None, None, outer) and ops.DANN_SINK is outer
    assert _sinks() == (None,) * 4
    with pytest.raises(TypeError):
        with ops.kinks(masks=True):
            pass
    with pytest.raises(TypeError):
        with ops.kinks(mask=False):
            pass
    assert _sinks() == (None,) * 4


def test_oracle_pinned_installs_restores_and_nests():
    km, inner = O.KinkMasks([]), O.KinkMasks([])
    assert O.KINK_MASKS is None
    with O.pinned(None):                                                # the unpinned mode: a no-op block
        assert O.KINK_MASKS is None
    with pytest.raises(ZeroDivisionError):
        with O.pinned(km):
            assert O.KINK_MASKS is km
            1 / 0
    assert O.KINK_MASKS is None                                         # restored on exception
    with O.pinned(km):
        with O.pinned(None):
            assert O.KINK_MASKS is None
        assert O.KINK_MASKS is km                                       # a nested pinned(None) restores the outer masks
        with O.pinned(inner):
            assert O.KINK_MASKS is inner
        assert O.KINK_MASKS is km
    assert O.KINK_MASKS is None


def test_parity_pinned_audits_what_the_oracle_consumed():
    from tests import parity
    x = torch.tensor([[1.0, -2.0], [0.5, -0.25]], dtype=torch.float64)
    with parity.pinned(O.KinkMasks([x > 0]), "agrees") as audit:        # every mask consumed, every branch the oracle's own
        y = O.activation(x, "relu")
    assert torch.equal(y, x.clamp_min(0)) and audit.worst_rel == 0.0 and audit.disagree_frac == 0.0
    assert O.KINK_MASKS is None
    with pytest.raises(AssertionError, match="fewer activations"):      # one recorded mask left over: done()
        with parity.pinned(O.KinkMasks([x > 0, x > 0]), "left over"):
            O.activation(x, "relu")
    flipped = x > 0
    flipped[0, 1] = True                                                # the recorded branch is wrong where |x| is the tensor's maximum
    with pytest.raises(AssertionError, match="pre-activation of real size"):
        with parity.pinned(O.KinkMasks([flipped]), "flipped") as audit:
            O.activation(x, "relu")
    assert audit.worst_rel == 1.0 and audit.disagree_frac == 0.25 and O.KINK_MASKS is None
    with parity.pinned(O.KinkMasks([flipped]), "reported, not asserted", check=False) as audit:
        O.activation(x, "relu")
    assert audit.worst_rel == 1.0
    with pytest.raises(ZeroDivisionError):                              # a block that raises is not audited; the masks still leave
        with parity.pinned(O.KinkMasks([x > 0, x > 0])):
            1 / 0
    assert O.KINK_MASKS is None
    with parity.pinned(None) as audit:                                  # no masks: no pinning, no audit
        assert O.KINK_MASKS is None


# ---- the pooling table of munit_amd.ops ------------------------------------------------------------------------------------
def test_pooling_table_names_every_pool_symbol_once_and_the_two_winner_channels():
    from munit_amd import _lib, ops
    assert sorted(ops._POOLS) == ["avgpool16", "avgpool3s2", "avgpool7", "global_avgpool", "maxpool2", "maxpool3s2"]
    assert all(callable(getattr(ops, name)) for name in ops._POOLS)      # keyed by the public functions' names
    named = [s for p in ops._POOLS.values() for s in (p.fwd, p.bwd)]
    want = [s for s in _lib.SIGNATURES if fnmatch.fnmatchcase(s, "munit_*pool*") or fnmatch.fnmatchcase(s, "munit_gap_*")]
    assert len(want) == 12 and sorted(named) == sorted(want) and len(set(named)) == 12
    assert all(p.fwd.endswith("_fwd") and p.bwd == p.fwd[:-3] + "bwd" for p in ops._POOLS.values())
    # a channel is held by NAME: the lists behind SEG_SINK / DANN_SINK exist only while ops.kinks is active
    assert {n: p.sink for n, p in ops._POOLS.items() if p.sink is not None} == {"maxpool3s2": "seg", "maxpool2": "dann"}
    assert ops._POOLS["maxpool2"].check is not None and [n for n, p in ops._POOLS.items() if p.check] == ["maxpool2"]
    with pytest.raises(RuntimeError, match=r"munit_amd.maxpool2: needs H, W >= 2 and C % 4 == 0, got \(1, 6, 4, 4\)"):
        ops._POOLS["maxpool2"].check(torch.Size((1, 6, 4, 4)))
    ops._POOLS["maxpool2"].check(torch.Size((1, 4, 2, 2)))
    assert ops._POOLS["avgpool3s2"].extent(5, 7) == (3, 4) and ops._POOLS["maxpool3s2"].extent(1, 1) == (1, 1)
    assert ops._POOLS["maxpool2"].extent(5, 3) == (2, 1) and ops._POOLS["global_avgpool"].extent(3, 5) == (1, 1)
    assert [n for n, p in ops._POOLS.items() if p.flat] == ["global_avgpool"]
