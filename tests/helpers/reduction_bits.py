"""The case behind tests/golden/p02_reduction_bits.npz: the raw record words of the three multi-tensor reductions whose float64
sums depend on the order of their additions - the statistics (`locate_stats_reduce`), the dynamics (`locate_dyn_pass`, modes 1
and 3) and the guard's verdict (`locate_guarded_nadam_step` with clipping on) - recorded by tools/record_reduction_bits.py and
compared word for word by tests/test_gpu_reduction_bits.py.  The fixture is this project's own output at one commit: it pins the
order of every addition (a thread's elements, the butterfly, the four waves, the partials) against later changes of the source.

Tensors of 1, 3, 4095, 4096, 4097 and 3 * 4096 + 2 elements, each once at a 16-byte-aligned base and once one element past one;
the dynamics add two pairs whose weight and base differ in alignment.  Magnitudes spread over 40 binades; one NaN and one Inf in
the statistics' and the guard's inputs; a dynamics base that differs from the weights in every third element.  Everything comes
from one seeded numpy generator: the fixture holds records only."""
import numpy as np
import torch

SIZES = (1, 3, 4095, 4096, 4097, 3 * 4096 + 2)
LAYOUT = [(n, off) for n in SIZES for off in (0, 1)]          # (elements, elements past a 16-byte boundary)
MIXED = [(4097, 0, 1), (4095, 1, 0)]          # dynamics only: (elements, offset of w, offset of base)
SEED = 20261020
MAX_NORM = 1.0
KEYS = ("stats/words", "dyn/mode1", "dyn/mode3", "guard/verdict")


def normals(rng, n):
    """mixed signs, magnitudes over 40 binades (tests/test_gpu_stats.py::normals)"""
    return (rng.standard_normal(n) * 2.0 ** rng.uniform(-20, 20, size=n)).astype(np.float32)


def inputs():
    """(x, w, base): lists of float32 numpy arrays - x for the statistics and the guard, in LAYOUT order, with one NaN and one
    Inf; w and base for the dynamics, in LAYOUT + MIXED order, base[i] != w[i] exactly where i % 3 == 1"""
    rng = np.random.default_rng(SEED)
    x = [normals(rng, n) for n, _ in LAYOUT]
    x[8][4096] = np.float32(np.nan)          # 4097 elements, aligned: the second chunk's only element
    x[11][2 * 4096 + 5] = np.float32(-np.inf)          # 3 * 4096 + 2 elements, one element past alignment
    w, base = [], []
    for n in [n for n, _ in LAYOUT] + [n for n, _, _ in MIXED]:
        a = normals(rng, n)
        b = a.copy()
        b[1::3] = normals(rng, len(b[1::3]))
        w.append(a)
        base.append(b)
    return x, w, base


def place(values, offset, dev):
    """`values` on the device, starting `offset` elements past a 16-byte boundary; the words around it are zero"""
    buf = torch.zeros(len(values) + 8, dtype=torch.float32, device=dev)
    view = buf[offset:offset + len(values)]
    view.copy_(torch.as_tensor(values))
    assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
    return view


def run(dev):
    """{key: int64 numpy array} for every key of KEYS"""
    from locate_amd import dynamics as D
    from locate_amd import stats as S
    from locate_amd.guard import GuardedNadam
    x, w, base = inputs()
    out = {}

    xs = [place(a, off, dev) for a, (_, off) in zip(x, LAYOUT)]
    row = torch.zeros(1 + len(xs), 2, dtype=torch.int64, device=dev)          # the summary, then the 16-byte records
    S._launch(S._device_table(xs), row)
    out["stats/words"] = row.cpu().numpy().copy()

    offsets = [(off, off) for _, off in LAYOUT] + [(ow, ob) for _, ow, ob in MIXED]
    ws = [place(a, ow, dev) for a, (ow, _) in zip(w, offsets)]
    bs = [place(b, ob, dev) for b, (_, ob) in zip(base, offsets)]
    table = D._device_table(ws, bs)
    for key, mode in (("dyn/mode1", D.RECORD), ("dyn/mode3", D.RECORD | D.REBASE)):          # mode 3 last: it rewrites the bases
        rec = torch.zeros(len(ws), D.WORDS, dtype=torch.int64, device=dev)
        D._launch(table, mode, rec)
        out[key] = rec.cpu().numpy().copy()
    for a, b in zip(ws, bs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "mode 3 leaves base == w bit for bit"

    ps = [torch.nn.Parameter(torch.zeros(n, dtype=torch.float32, device=dev)) for n, _ in LAYOUT]
    for p, g in zip(ps, xs):
        p.grad = g
    opt = GuardedNadam(ps, max_norm=MAX_NORM, skip_nonfinite=False)          # the scale comes from the sums, NaN or not
    opt.step()
    torch.cuda.synchronize()
    out["guard/verdict"] = opt._verdict.cpu().numpy().copy()          # the 64-byte record
    assert set(out) == set(KEYS)
    return out
