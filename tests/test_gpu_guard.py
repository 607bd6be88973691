"""The guarded Nadam step on the MI355X (locate_amd/guard.py, csrc/guard.hip), bit for bit against what is not the code under test:
`Nadam` itself (an idle guard; a clipped step against Nadam on gradients premultiplied by the device's own scale; the step behind
a skipped one), the float64 model of the norm and the verdict (tests/helpers/stats_model.py, guard_model.py), and the state a
skipped step has to leave alone - eagerly, inside a captured graph where the decision is taken at replay time, and inside a
training run of the tiny fixture network."""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import guard_model as GM  # noqa: E402
import stats_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
CHUNK = 4096
SIZES = [1, 3, 4095, 4096, 4097, 8193, 40000]          # tests/test_gpu_amax.py's Nadam sizes: they straddle one and two chunk edges
VIEW_N = 5001                                          # ... a view one element into a larger buffer: 4-byte alignment only
UNUSED_N = 77                                          # ... and a parameter whose .grad is None
FIRST, N4097, ONE, VIEW = 0, SIZES.index(4097), SIZES.index(1), len(SIZES)


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def host_weights():
    rng = np.random.default_rng(100)
    return tuple(rng.standard_normal(n).astype(np.float32) for n in SIZES + [VIEW_N, UNUSED_N])


@functools.lru_cache(maxsize=None)
def host_grads(step):
    """one gradient per parameter that has one: mixed signs, magnitudes over 16 binades"""
    rng = np.random.default_rng(200 + step)
    return tuple((rng.standard_normal(n) * 2.0 ** rng.uniform(-8, 8, size=n)).astype(np.float32) for n in SIZES + [VIEW_N])


@functools.lru_cache(maxsize=None)
def model_statistics(step):
    """(sumsq, nonfinite, n) of host_grads(step) by the model - computed once"""
    return GM.global_statistics(host_grads(step))


class Rig:
    """The parameters above under one optimizer with two parameter groups (another learning rate in the second).  Parameters and
    gradients live in buffers that keep their addresses, so a captured step finds them again."""

    def __init__(self, cls, weight_decay=0.0, **kw):
        self.keep, self.params, self.grads = [], [], []
        for i, w in enumerate(host_weights()):
            n = w.size
            if i == VIEW:
                buf, gbuf = torch.zeros(n + 7, device=DEV), torch.zeros(n + 7, device=DEV)
                self.keep += [buf, gbuf]
                p, g = torch.nn.Parameter(buf[1:1 + n]), gbuf[1:1 + n]
                assert p.data_ptr() % 16 == 4 and g.data_ptr() % 16 == 4 and p.is_contiguous()
            else:
                p = torch.nn.Parameter(torch.zeros(n, 1, device=DEV) if i % 2 == 0 else torch.zeros(n, device=DEV))
                g = torch.zeros_like(p) if i != VIEW + 1 else None
            with torch.no_grad():
                p.copy_(T(w).view_as(p))
            p.grad = g
            self.params.append(p)
            self.grads.append(g)
        groups = [{"params": self.params[:4]}, {"params": self.params[4:], "lr": 5e-4}]
        self.opt = cls(groups, lr=2e-3, weight_decay=weight_decay, **kw)

    def set_grads(self, grads, scale=None):
        for g, h in zip(self.grads, grads):
            g.copy_(T(h).view_as(g))
            if scale is not None:
                g.mul_(torch.tensor(scale, dtype=torch.float32, device=DEV))          # one fp32 multiplication per element
        return self

    def poison(self, which, where, value):
        self.grads[which].view(-1)[where] = value

    def step(self):
        self.opt.step()
        return self

    def state(self):
        """every bit a step may touch, as integers: NaN compares by its pattern"""
        torch.cuda.synchronize()
        out = {}
        for i, p in enumerate(self.params):
            out["p%d" % i] = p.detach().view(torch.int32).clone()
            for k, v in self.opt.state.get(p, {}).items():
                out["%s%d" % (k, i)] = v.view(torch.int64 if v.dtype == torch.float64 else torch.int32).clone()
            hold = p.__dict__.get("_locate_wmax")
            if hold is not None:
                out["absmax%d" % i] = hold[0].clone()
                out["stamp%d" % i] = torch.tensor([hold[1] - p._version])
        return out

    def grad_bits(self):
        torch.cuda.synchronize()
        return [g.view(torch.int32).clone() for g in self.grads if g is not None]


def differing(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


def assert_words_hold_the_weights(rig, what):
    for i, p in enumerate(rig.params):
        hold = p.__dict__.get("_locate_wmax")
        if hold is None:
            assert rig.grads[i] is None
            continue
        assert hold[1] == p._version, "%s: parameter %d stamp %d, version %d" % (what, i, hold[1], p._version)
        got, want = int(hold[0].max()), int(p.detach().abs().max().reshape(1).view(torch.int32))
        assert int(hold[0].min()) >= 0 and got == want, "%s: parameter %d words %#010x, weights %#010x" % (what, i, got, want)


# ---- 1. idle is Nadam ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_idle_is_nadam(weight_decay):
    from locate_amd import GuardedNadam, Nadam
    plain = Rig(Nadam, weight_decay)
    guarded = {"max_norm 0": Rig(GuardedNadam, weight_decay, max_norm=0.0), "max_norm 1e30": Rig(GuardedNadam, weight_decay, max_norm=1e30)}
    for step in range(5):
        want = plain.set_grads(host_grads(step)).step().state()
        assert any(k.startswith("absmax") for k in want) and any(k.startswith("sched") for k in want)
        for name, rig in guarded.items():
            bad = differing(want, rig.set_grads(host_grads(step)).step().state())
            assert not bad, "%s, weight decay %g, step %d: %s differ from Nadam" % (name, weight_decay, step, bad)
    for name, rig in guarded.items():
        c = rig.opt.counters()
        assert (c["steps"], c["skipped"], c["clipped"], c["consecutive_skips"], c["last_nonfinite"]) == (5, 0, 0, 0, 0), name
        assert c["last_scale"] == 1.0 and c["last_norm"] > 0
        assert rig.params[VIEW + 1].grad is None and rig.params[VIEW + 1] not in rig.opt.state          # the unused one was passed over
        assert torch.equal(rig.params[VIEW + 1].detach().cpu().view(-1), T(host_weights()[VIEW + 1]))
    assert_words_hold_the_weights(guarded["max_norm 0"], "idle")


# ---- 2. the norm -----------------------------------------------------------------------------------------------------------------
def test_norm_against_the_model():
    from locate_amd import GuardedNadam
    rig = Rig(GuardedNadam)
    for step in (0, 1):
        c = rig.set_grads(host_grads(step)).step().opt.counters()
        want, nonfinite, n = model_statistics(step)
        got = c["last_norm"] ** 2
        print("step %d: n %d  norm^2 %.17g  model %.17g  rel %.3g (bound %.3g)" % (step, n, got, want, abs(got - want) / want, M.sumsq_tolerance(n)))
        assert nonfinite == 0 and c["last_nonfinite"] == 0 and n == sum(SIZES) + VIEW_N
        assert M.sumsq_close(got, want, n)
    again = Rig(GuardedNadam).set_grads(host_grads(1)).step().opt.counters()          # the same gradients at other addresses of the same alignment
    assert again["last_norm"] == c["last_norm"]


def test_more_chunks_than_the_reduce_grid():
    """one gradient of more chunks than the reduce kernel has blocks: ones, with a 2.0, a 1e30 and (second step) a NaN in chunks that
    only the second grid-stride round reaches; the terms of the model's sum are exact"""
    from locate_amd import GuardedNadam, Nadam
    from locate_amd._lib import lib
    cap = lib().locate_guard_max_blocks()
    assert 0 < cap <= 4096 and lib().locate_guard_chunk_elems() == CHUNK
    n = (cap + 3) * CHUNK + 5
    two, huge, nan = (cap + 1) * CHUNK + 7, n - 1, (cap + 2) * CHUNK + 4095
    torch.manual_seed(3)
    start = torch.randn(n, device=DEV)
    rigs = []
    for cls in (GuardedNadam, Nadam):
        p = torch.nn.Parameter(start.clone())
        p.grad = torch.ones(n, device=DEV)
        p.grad[two], p.grad[huge] = 2.0, 1e30
        rigs.append((p, cls([p], lr=2e-3)))
    (p, opt), (q, ref) = rigs
    opt.step()
    ref.step()
    torch.cuda.synchronize()
    c = opt.counters()
    want = math.fsum([float(n - 2), 4.0, float(np.float32(1e30)) ** 2])
    got = c["last_norm"] ** 2
    print("n %d  norm^2 %.17g  model %.17g  rel %.3g (bound %.3g)" % (n, got, want, abs(got - want) / want, M.sumsq_tolerance(n)))
    assert M.sumsq_close(got, want, n) and c["last_nonfinite"] == 0 and c["skipped"] == 0
    assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
    for k in ("exp_avg", "exp_avg_sq", "sched"):
        assert torch.equal(opt.state[p][k], ref.state[q][k]), k
    assert torch.equal(p.__dict__["_locate_wmax"][0], q.__dict__["_locate_wmax"][0])
    p.grad[huge], p.grad[nan] = 1.0, float("nan")
    before = p.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    c = opt.counters()
    assert (c["last_nonfinite"], c["skipped"], c["steps"]) == (1, 1, 2)
    assert c["last_norm"] ** 2 == float(n + 2)          # n - 2 ones and one 4: every partial sum is an integer below 2^53
    assert torch.equal(p.detach(), before)


# ---- 3. clipping -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_clip(weight_decay):
    from locate_amd import GuardedNadam, Nadam
    sumsq, _, n = model_statistics(0)
    norm_model = math.sqrt(sumsq)
    max_norm = 0.5 * norm_model
    rig, ref = Rig(GuardedNadam, weight_decay, max_norm=max_norm), Rig(Nadam, weight_decay)
    rig.set_grads(host_grads(0))
    before = rig.grad_bits()
    c = rig.step().opt.counters()
    want = np.float32(np.float64(max_norm) / np.float64(norm_model))
    print("scale %.9g (bits %#010x), model %.9g" % (c["last_scale"], int(np.array([c["last_scale"]], np.float32).view(np.uint32)[0]), want))
    assert GM.scale_within_one_ulp(c["last_scale"], want)
    assert (c["clipped"], c["skipped"], c["steps"]) == (1, 0, 1)
    assert all(torch.equal(a, b) for a, b in zip(before, rig.grad_bits())), ".grad was written"
    # Nadam on gradients premultiplied, in fp32, by the scale the device took
    ref.set_grads(host_grads(0), scale=c["last_scale"]).step()
    bad = differing(ref.state(), rig.state())
    assert not bad, "weight decay %g: %s differ from Nadam on premultiplied gradients" % (weight_decay, bad)
    # ... and not what Nadam gives on the gradients as they are
    assert differing(Rig(Nadam, weight_decay).set_grads(host_grads(0)).step().state(), rig.state())
    # a second step whose norm is below the limit: taken unscaled
    small = tuple(g * np.float32(2.0 ** -12) for g in host_grads(1))
    c = rig.set_grads(small).step().opt.counters()
    assert (c["clipped"], c["steps"], c["last_scale"]) == (1, 2, 1.0) and c["last_norm"] < max_norm
    assert not differing(ref.set_grads(small).step().state(), rig.state())


# ---- 4. skipping -------------------------------------------------------------------------------------------------------------------
PLACES = {"first of the first tensor": (FIRST, 0), "last of the 4097 tensor": (N4097, 4096), "the 1-element tensor": (ONE, 0),
          "first of the misaligned view": (VIEW, 0), "last of the misaligned view": (VIEW, VIEW_N - 1)}


@pytest.mark.parametrize("place", list(PLACES))
def test_skip(place):
    from locate_amd import GuardedNadam, Nadam
    which, where = PLACES[place]
    rig, ref = Rig(GuardedNadam), Rig(Nadam)
    taken, ref_taken = Rig(GuardedNadam, skip_nonfinite=False), Rig(Nadam)
    for r in (rig, ref, taken, ref_taken):
        r.set_grads(host_grads(0)).step()          # one clean step: moments and schedule are not their initial values
    kept = rig.state()
    assert not differing(kept, ref.state())
    skipped = 0
    for step, value in enumerate((float("nan"), float("inf"), -float("inf")), start=1):
        what = "%s, %r" % (place, value)
        rig.set_grads(host_grads(step)).poison(which, where, value)
        after = rig.step().state()
        skipped += 1
        bad = [k for k in differing(kept, after) if not k.startswith(("absmax", "stamp"))]
        assert not bad, "%s: a skipped step changed %s" % (what, bad)
        assert_words_hold_the_weights(rig, what)
        c = rig.opt.counters()
        assert (c["skipped"], c["consecutive_skips"], c["last_nonfinite"], c["last_scale"]) == (skipped, 1, 1, 1.0), (what, c)
        # the next step, with clean gradients, is Nadam's step from the state before the skip
        c = rig.set_grads(host_grads(step)).step().opt.counters()
        kept = rig.state()
        bad = differing(ref.set_grads(host_grads(step)).step().state(), kept)
        assert not bad, "%s: the step behind the skipped one differs from Nadam in %s" % (what, bad)
        assert (c["skipped"], c["consecutive_skips"], c["last_nonfinite"], c["steps"]) == (skipped, 0, 0, 1 + 2 * step), (what, c)
        # skip_nonfinite=False: the step is taken, as Nadam takes it
        taken.set_grads(host_grads(step)).poison(which, where, value)
        ref_taken.set_grads(host_grads(step)).poison(which, where, value)
        bad = differing(ref_taken.step().state(), taken.step().state())
        assert not bad, "%s: skip_nonfinite=False differs from Nadam in %s" % (what, bad)
        c = taken.opt.counters()
        assert (c["skipped"], c["last_nonfinite"], c["steps"]) == (0, 1, 1 + step), (what, c)
    # two skipped steps in a row: the device counts them, and a clean step starts the count again
    kept = rig.state()
    for k in (1, 2):
        rig.set_grads(host_grads(4)).poison(which, where, float("nan"))
        rig.poison(FIRST, 0, float("inf"))
        bad = [n for n in differing(kept, rig.step().state()) if not n.startswith(("absmax", "stamp"))]
        c = rig.opt.counters()
        assert not bad and (c["skipped"], c["consecutive_skips"]) == (skipped + k, k), (place, k, bad, c)
        assert c["last_nonfinite"] == (1 if (which, where) == (FIRST, 0) else 2)
    c = rig.set_grads(host_grads(4)).step().opt.counters()
    assert (c["skipped"], c["consecutive_skips"]) == (skipped + 2, 0)
    assert not differing(ref.set_grads(host_grads(4)).step().state(), rig.state())
    assert not bool(torch.isfinite(taken.params[which]).all())          # the poison did reach the weights there
    assert all(bool(torch.isfinite(p).all()) for p in rig.params)


# ---- 5. inside a graph -----------------------------------------------------------------------------------------------------------
def test_inside_a_graph():
    from locate_amd import GuardedNadam, Nadam
    rig, ref = Rig(GuardedNadam, max_norm=1e30), Rig(Nadam)
    rig.set_grads(host_grads(0)).step()          # eagerly once: the tables and the record exist before the capture
    ref.set_grads(host_grads(0)).step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rig.opt.step()
    assert not differing(ref.state(), rig.state())          # a capture runs nothing

    def replay():
        graph.replay()
        torch._C._increment_version([p for p, g in zip(rig.params, rig.grads) if g is not None])          # as GraphedTrainStep.replay does
        for p in rig.params:
            hold = p.__dict__.get("_locate_wmax")
            if hold is not None:
                hold[1] = p._version
        return rig.state()

    rig.set_grads(host_grads(1))
    bad = differing(ref.set_grads(host_grads(1)).step().state(), replay())
    assert not bad, "clean replay: %s differ from Nadam" % bad
    kept = rig.state()
    rig.set_grads(host_grads(2)).poison(N4097, 4096, float("nan"))
    rig.poison(VIEW, 0, float("inf"))
    after = replay()
    bad = [k for k in differing(kept, after) if not k.startswith(("absmax", "stamp"))]
    assert not bad, "poisoned replay changed %s" % bad
    assert_words_hold_the_weights(rig, "poisoned replay")
    c = rig.opt.counters()
    assert (c["steps"], c["skipped"], c["consecutive_skips"], c["last_nonfinite"]) == (3, 1, 1, 2)
    rig.set_grads(host_grads(2))
    bad = differing(ref.set_grads(host_grads(2)).step().state(), replay())
    assert not bad, "clean replay behind the poisoned one: %s differ from Nadam" % bad
    c = rig.opt.counters()
    assert (c["steps"], c["skipped"], c["consecutive_skips"], c["last_nonfinite"], c["clipped"]) == (4, 1, 0, 0, 0)


def test_first_step_inside_a_capture_is_refused():
    """the counter record must exist before a capture: a captured zero fill would reset the counters at every replay"""
    from locate_amd import GuardedNadam
    rig = Rig(GuardedNadam).set_grads(host_grads(0))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="before a stream capture"):
        with torch.cuda.graph(graph):
            rig.opt._record(DEV)
    assert rig.opt._verdict is None and rig.opt.counters() == GM.ZERO


# ---- 6. in a run: the tiny fixture network of tests/test_gpu_stats.py (32 x 32, base width 1, batch 8) -----------------------------
def build_tiny(make_opt):
    from locate_amd import Discriminator, Generator, NetConfig, TrainStep
    z = load_golden("g8_tiny_e2e")
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    G.load_state_dict({k[len("G/sd0/"):]: T(z[k]) for k in z.files if k.startswith("G/sd0/")})
    D.load_state_dict({k[len("D/sd0/"):]: T(z[k]) for k in z.files if k.startswith("D/sd0/")})
    G.noise = T(z["G/noise"])
    G, D = G.to(DEV), D.to(DEV)
    G.batched_spectral_norm = D.batched_spectral_norm = True
    step = TrainStep(G, D, make_opt("G", G.parameters(), lr=cfg.glr, betas=(cfg.beta1, cfg.beta2)),
                     make_opt("D", D.parameters(), lr=cfg.dlr, betas=(cfg.beta1, cfg.beta2)), stacked_d=True, minibatches=1)
    inputs = tuple(T(z["step1/" + k]).to(DEV) for k in ("latent", "real", "aug"))
    return G, D, step, inputs


def training_state(G, D, step):
    """every parameter (u and v included) and every Nadam state tensor, by name"""
    torch.cuda.synchronize()
    state = {"G/" + k: v.detach().clone() for k, v in G.state_dict().items()}
    state.update({"D/" + k: v.detach().clone() for k, v in D.state_dict().items()})
    for tag, net, opt in (("G", G, step.gen_opt), ("D", D, step.dis_opt)):
        for name, q in net.named_parameters():
            for k, v in opt.state.get(q, {}).items():
                if torch.is_tensor(v):
                    state["%s/opt/%s/%s" % (tag, name, k)] = v.detach().clone()
    return state


def nadam_factory(tag, params, **kw):
    from locate_amd import Nadam
    return Nadam(params, **kw)


def guarded_factory(max_norms):
    def make(tag, params, **kw):
        from locate_amd import GuardedNadam
        return GuardedNadam(params, max_norm=max_norms[tag], **kw)
    return make


REPLAYS = 4


def run_tiny(make_opt, launch_mode):
    """two iterations and REPLAYS more - eagerly, or the two as GraphedTrainStep's warm-up and the rest as replays; returns the
    final state, both optimizers' counters (None for Nadam) and the first iteration's"""
    from locate_amd.graph import GraphedTrainStep
    G, D, step, (lat, real, aug) = build_tiny(make_opt)
    read = lambda: {tag: opt.counters() if hasattr(opt, "counters") else None for tag, opt in (("G", step.gen_opt), ("D", step.dis_opt))}  # noqa: E731
    first = None
    if launch_mode == "graphed":
        runner = GraphedTrainStep(step, lat, real, aug, warmup=2)
        for _ in range(REPLAYS):
            runner.replay()
    else:
        for i in range(2 + REPLAYS):
            step(lat, real, aug)
            if i == 0:
                first = read()
    return training_state(G, D, step), read(), first


@functools.lru_cache(maxsize=None)
def idle_eager_run():
    return run_tiny(guarded_factory({"G": 0.0, "D": 0.0}), "eager")


@pytest.mark.parametrize("launch_mode", ["eager", "graphed"])
def test_idle_run_is_the_nadam_run(launch_mode):
    plain, _, _ = run_tiny(nadam_factory, launch_mode)
    guarded, counters, _ = idle_eager_run() if launch_mode == "eager" else run_tiny(guarded_factory({"G": 0.0, "D": 0.0}), launch_mode)
    assert sorted(plain) == sorted(guarded)
    bad = [k for k in plain if not torch.equal(plain[k], guarded[k])]
    assert not bad, "%s: %d of %d tensors differ, first %s" % (launch_mode, len(bad), len(plain), bad[:4])
    assert any(k.endswith("weight_u") for k in plain) and any("/opt/" in k for k in plain)
    for tag in ("G", "D"):
        c = counters[tag]
        assert (c["steps"], c["skipped"], c["clipped"], c["last_scale"]) == (2 + REPLAYS, 0, 0, 1.0) and c["last_norm"] > 0, (launch_mode, tag, c)


def test_clipped_replay_equals_the_eager_clipped_run():
    _, _, first = idle_eager_run()
    max_norms = {tag: 0.25 * first[tag]["last_norm"] for tag in ("G", "D")}          # below the first iteration's recorded norm
    assert all(v > 0 and math.isfinite(v) for v in max_norms.values())
    eager, c_eager, c_first = run_tiny(guarded_factory(max_norms), "eager")
    graphed, c_graphed, _ = run_tiny(guarded_factory(max_norms), "graphed")
    bad = [k for k in eager if not torch.equal(eager[k], graphed[k])]
    assert sorted(eager) == sorted(graphed) and not bad, "%d of %d tensors differ, first %s" % (len(bad), len(eager), bad[:4])
    print("first iteration: %r\nlast: %r" % (c_first, c_eager))
    for tag in ("G", "D"):
        assert c_first[tag]["clipped"] == 1 and c_first[tag]["last_scale"] < 1.0
        assert c_eager[tag] == c_graphed[tag] and c_eager[tag]["clipped"] > 0 and c_eager[tag]["skipped"] == 0
    assert c_first["D"]["last_norm"] == first["D"]["last_norm"]          # the first discriminator step sees the idle run's gradients
    idle, _, _ = idle_eager_run()
    assert any(not torch.equal(idle[k], eager[k]) for k in idle)          # the clipping did change the run


def test_a_poisoned_discriminator_gradient_costs_one_step():
    G, D, step, (lat, real, aug) = build_tiny(guarded_factory({"G": 0.0, "D": 0.0}))
    for _ in range(2):
        step(lat, real, aug)
    step.d_forward_backward(lat, real, aug)
    kept = training_state(G, D, step)
    name, weight = next((n, p) for n, p in D.named_parameters() if p.grad is not None and p.numel() > 16)
    weight.grad.view(-1)[11] = float("nan")
    step.d_optimizer()
    after = training_state(G, D, step)
    bad = [k for k in kept if not torch.equal(kept[k], after[k])]
    assert sorted(kept) == sorted(after) and not bad, "the skipped step changed %s" % bad[:4]
    c = step.dis_opt.counters()
    assert (c["steps"], c["skipped"], c["consecutive_skips"], c["last_nonfinite"]) == (3, 1, 1, 1)
    step.g_step(lat)
    step(lat, real, aug)          # the following iteration
    final = training_state(G, D, step)
    assert all(bool(torch.isfinite(v).all()) for v in final.values() if v.is_floating_point())
    moved = [k for k in kept if k.startswith("D/") and not torch.equal(kept[k], final[k])]
    assert len(moved) >= 10, "the discriminator did not train on"
    c = step.dis_opt.counters()
    assert (c["steps"], c["skipped"], c["consecutive_skips"]) == (4, 1, 0) and step.gen_opt.counters()["skipped"] == 0


# ---- 7. bad arguments ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    from locate_amd._lib import lib
    L = lib()
    buf = torch.zeros(256, dtype=torch.uint8, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    odd = ctypes.c_void_p(buf.data_ptr() + 4)
    hyper = (2e-3, 0.9, 0.999, 1e-8, 4e-3, 0.0, None)
    #        grads chunks n_g n_gc ws verdict max_norm skip | tensors coef chunks n_t n_c
    good = [p, p, 1, 1, p, p, 0.0, 1, p, p, p, 1, 1]
    cases = []
    for at, value in ((0, None), (1, None), (4, None), (5, None), (8, None), (9, None), (10, None),          # null tables and buffers
                      (2, -1), (3, 0), (3, -2), (11, 0), (11, -1), (12, 0), (12, -3),                         # zero and negative counts
                      (5, odd), (4, odd),                                                                     # misaligned record buffers
                      (6, -1.0), (6, float("nan")), (6, float("inf"))):                                      # max_norm
        args = list(good)
        args[at] = value
        cases.append(args)
    cases.append([p, p, 0, 0, p, p, 0.0, 1, p, p, p, 1, 1])          # no gradient count, but a gradient table
    cases.append([None, None, 0, 1, None, p, 0.0, 1, p, p, p, 1, 1])
    cases.append([None, None, 0, 0, odd, p, 0.0, 1, p, p, p, 1, 1])
    for args in cases:
        assert L.locate_guarded_nadam_step(*args, *hyper) == 1, args
        assert b"locate_guarded_nadam_step" in L.locate_last_error()
    torch.cuda.synchronize()
    assert not buf.any()          # nothing was launched: every table above is zeros, and a verdict would have counted a step
    assert L.locate_guard_verdict_bytes() == 64 and L.locate_guard_tensor_record_bytes() == 16
    assert L.locate_guard_workspace_bytes(3) == 48 and L.locate_guard_workspace_bytes(0) == 0


# ---- 8. trainer, resume, command line ----------------------------------------------------------------------------------------------
def test_trainer_and_resume(tmp_path):
    from locate_amd import DeviceImageStore, GuardedNadam, InputPipeline, Trainer
    images = np.random.default_rng(6).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)

    def trainer(out, max_iterations, guarded=True):
        _, _, step, _ = build_tiny(guarded_factory({"G": 1e-6, "D": 1e-6}) if guarded else nadam_factory)
        pipeline = InputPipeline(store, 32, 8, seed=11)
        return Trainer(step, pipeline, str(out), epochs=2, max_iterations=max_iterations, images=13, seed=3, miniter_function=lambda e: 1,
                       subepoch_function=lambda e: 1, image_interval_function=lambda batch: 2)

    def files(out):
        return sorted(os.path.relpath(os.path.join(d, f), str(out)) for d, _, fs in os.walk(str(out)) for f in fs)

    out = tmp_path / "on"
    t = trainer(out, 4)
    assert t.run() == 4
    with open(str(out / "error" / "1-guard.json")) as f:
        record = json.load(f)
    assert sorted(record) == ["D", "G"] and all(sorted(record[k]) == sorted(GM.ZERO) for k in record)
    assert all((record[k]["steps"], record[k]["skipped"], record[k]["clipped"]) == (4, 0, 4) for k in record)
    assert str(out / "error" / "1-guard.json") in t.written and not os.path.exists(str(out / "error" / "nonfinite.json"))
    saved = torch.load(str(out / "trainer.torch"), map_location="cpu", weights_only=True)
    assert saved["guard"] == {"G": t.step.gen_opt.counters(), "D": t.step.dis_opt.counters()} and saved["guard"]["G"]["steps"] == 4
    # without guarded optimizers: the same files but the guard's, and no key of its
    plain = trainer(tmp_path / "off", 4, guarded=False)
    assert plain.run() == 4
    assert [f for f in files(out) if f != os.path.join("error", "1-guard.json")] == files(tmp_path / "off")
    assert "guard" not in torch.load(str(tmp_path / "off" / "trainer.torch"), map_location="cpu", weights_only=True)
    assert sorted(k for k in saved if k != "guard") == sorted(torch.load(str(tmp_path / "off" / "trainer.torch"), map_location="cpu", weights_only=True))
    # a resumed run counts on
    fresh = trainer(out, 6)
    assert isinstance(fresh.step.dis_opt, GuardedNadam) and fresh.resume().iterations == 4
    assert fresh.step.dis_opt.counters() == saved["guard"]["D"] and fresh.step.gen_opt.counters() == saved["guard"]["G"]
    assert fresh.run() == 6
    for opt in (fresh.step.gen_opt, fresh.step.dis_opt):
        c = opt.counters()
        assert (c["steps"], c["clipped"], c["skipped"]) == (6, 6, 0)
    # a trainer.torch without counters (a run that was not guarded) resumes with counters at zero
    fresh = trainer(tmp_path / "off", 6)
    assert fresh.resume().iterations == 4 and fresh.step.dis_opt.counters() == GM.ZERO


def test_command_line_flags(tmp_path):
    store = str(tmp_path / "store.npy")
    np.save(store, np.random.default_rng(8).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8))
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--batch", "8", "--out", out, "--epochs", "1",
           "--minibatches", "1", "--images", "16", "--clip-grad-norm", "1e-6", "--max-iterations", "4"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "4 iterations" in done.stdout
    with open(os.path.join(out, "error", "1-guard.json")) as f:
        record = json.load(f)
    assert sorted(record) == ["D", "G"]
    assert all((record[k]["steps"], record[k]["skipped"], record[k]["clipped"]) == (4, 0, 4) and record[k]["last_scale"] < 1.0 for k in record)
    assert not os.path.exists(os.path.join(out, "error", "nonfinite.json"))
    assert "guard" in torch.load(os.path.join(out, "trainer.torch"), map_location="cpu", weights_only=True)
