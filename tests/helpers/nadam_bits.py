"""The case behind tests/golden/p01_nadam_bits.npz: three `Nadam` steps whose every bit is recorded (tools/record_nadam_bits.py)
and compared (tests/test_gpu_ops.py::test_nadam_step_keeps_its_recorded_bits).  The fixture is this project's own output at one
commit: it pins the rounding of the update against later changes of the source and of the compiler.

Tensors of 1, 3, 4095 and 4097 elements (below, at and above one 4096-element chunk), a 4100-element parameter that starts one
element into a larger buffer (4-byte aligned only, its gradient likewise) and a parameter whose `.grad` is None.  The inputs come
from a seeded numpy generator; in every step one gradient element is exactly 0 and one is a denormal."""
import hashlib

import numpy as np
import torch

SIZES = (1, 3, 4095, 4097, 4100)          # the last one is the misaligned view
WEIGHT_DECAYS = (0.0, 0.01)
STEPS = 3
SEED = 20261019
HYPER = dict(lr=2e-3, betas=(0.5, 0.999), eps=1e-8, schedule_decay=4e-3)
KINDS = ("p", "exp_avg", "exp_avg_sq", "sched")


def inputs():
    """(initial parameters, gradients[step][tensor]) as float32 numpy arrays"""
    rng = np.random.default_rng(SEED)
    p0 = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    grads = []
    for _ in range(STEPS):
        gs = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32) for n in SIZES]
        gs[2][7] = np.float32(0.0)
        gs[3][4096] = np.float32(1e-41)          # a denormal, in the second chunk's only element
        grads.append(gs)
    return p0, grads


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run(weight_decay, dev):
    """{"step<s>/<kind><i>": numpy array} for s = 1 .. STEPS, plus "frame": the words around the misaligned parameter and the
    parameter without a gradient, which no step may touch"""
    from locate_amd import Nadam
    p0, grads = inputs()
    frame = torch.full((SIZES[-1] + 8,), 7.0, device=dev)
    ps = [torch.nn.Parameter(torch.as_tensor(a).to(dev)) for a in p0[:-1]]
    frame[1:1 + SIZES[-1]] = torch.as_tensor(p0[-1]).to(dev)
    ps.append(torch.nn.Parameter(frame[1:1 + SIZES[-1]]))
    idle = torch.nn.Parameter(torch.arange(5, dtype=torch.float32, device=dev))
    assert ps[-1].data_ptr() % 16 == 4 and ps[-1].is_contiguous()
    gframe = torch.zeros(SIZES[-1] + 8, device=dev)
    opt = Nadam(ps + [idle], weight_decay=weight_decay, **HYPER)
    out = {}
    for s in range(STEPS):
        for i, p in enumerate(ps[:-1]):
            p.grad = torch.as_tensor(grads[s][i]).to(dev)
        gframe[1:1 + SIZES[-1]] = torch.as_tensor(grads[s][-1]).to(dev)
        ps[-1].grad = gframe[1:1 + SIZES[-1]]
        opt.step()
        torch.cuda.synchronize()
        for i, p in enumerate(ps):
            st = opt.state[p]
            for kind, t in (("p", p), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"]), ("sched", st["sched"])):
                out["step%d/%s%d" % (s + 1, kind, i)] = t.detach().cpu().numpy().copy()
    assert len(opt.state.get(idle, {})) == 0
    out["frame"] = np.concatenate([frame[:1].cpu().numpy(), frame[1 + SIZES[-1]:].cpu().numpy(), idle.detach().cpu().numpy()])
    return out
