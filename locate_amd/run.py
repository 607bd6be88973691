"""The reference's outer loop (main.py:100-236) over `InputPipeline`, `TrainLoop` and the training monitor: epochs whose
schedule grows with the epoch number, sub-passes over the data, a sample picture every `image_intervall` iterations and at the
end of every pass, the loss curves and a checkpoint after every epoch.  Host glue only - everything it calls computes on the GPU.

    python -m locate_amd.run --store FILE.npy --image-size S --batch B --out DIR [--epochs N] [--max-iterations N]
                             [--images 64] [--seed 999] [--minibatches 8] [--diters 1] [--graph] [--resume] [--keep-spectral-norm]
                             [--swd-images 0] [--ema-half-life 0] [--stats-every 0] [--dynamics-every 0] [--formats-every 0]
                             [--clip-grad-norm X] [--no-skip-nonfinite] [--max-consecutive-skips 16]
                             [--rollback-every 0] [--max-rollbacks 3] [--spill-every 0] [--neighbours 0] [--neighbours-k 3]
                             [--manifold 0] [--manifold-k 3] [--spectrum-images 0] [--spectrum-window none]
                             [--msssim-pairs 0] [--modes 0] [--modes-bins 128] [--modes-images 16384]
                             [--diffaugment POLICY] [--ada-target X] [--ada-kimg 500] [--ada-interval 4] [--ada-initial-p 0]
                             [--ada-p-max 1] [--lecam WEIGHT] [--lecam-decay 0.99] [--lecam-warmup 1000] [--lecam-two-sided]
                             [--topk-floor F] [--topk-gamma 0.99] [--topk-every N]

Differences from the reference, all additions:
  * `--resume` / `Trainer.resume()`: the reference cannot continue a run.  Here `OUT/trainer.torch` (epoch, sub-pass, position,
    the input pipeline's state, the fixed latents, the latent generator's state, the loss history) and the checkpoint files of
    `locate_amd.checkpoint` are written after every epoch and whenever `max_iterations` stops the run, and a resumed run continues
    the uninterrupted one's trajectory;
  * the run ends after `epochs` epochs (the reference loops for ever) or after `max_iterations` iterations in all;
  * every iteration that steps the optimizers is recorded for the loss curves (a record is two small launches and no host read);
    the reference appends only the values it prints.  The progress line at `print_every` is the only place a loss is read on
    the host;
  * the per-iteration latents come from a generator of the trainer's own, so that its state can be saved;
  * `swd=` / `--swd-images N` (off by default): after every epoch the sliced Wasserstein distance of the generator against N
    real images (`locate_amd.metric`) is appended to `OUT/error/swd.json`.  The evaluation has no side effect on the training;
  * `average=` / `--ema-half-life IMAGES` (off by default): an exponential moving average of the generator's weights
    (`locate_amd.average`) whose weight of an old value halves every IMAGES images.  It is updated after every iteration by one
    launch beside the training step - the trajectory is untouched - and costs one more copy of the generator's parameters (plus
    its weight panels once it is sampled).  Its spectral-norm u / v are not averaged but copied from the live generator on every
    update.  Beside each picture `X.png` the average's picture of the same latents is written as `X.ema.png`, the metric's records
    gain an "average" entry, `OUT/netG_ema.torch` holds the averaged weights in the reference's `state_dict()` layout and
    `OUT/trainer.torch` the average's whole state, so a resumed run continues it.  Under data parallelism only rank 0 needs one;
  * `stats=` / `--stats-every N` (off by default): after every N-th iteration one record of per-tensor statistics - sum of
    squares, largest magnitude, number of non-finite elements of every weight and every gradient of both networks
    (`locate_amd.stats`) - is taken by a launch beside the training step; `OUT/error/{epoch}-stats.npz` holds an epoch's records.
    The records are checked wherever the losses are read and immediately before every save: a run that holds a NaN or an Inf
    stops with `NonFiniteError`, writes `OUT/error/nonfinite.json` and leaves the files of the last good save as they are;
  * `dynamics=` / `--dynamics-every N` (off by default): around every N-th iteration, per tensor the update-to-weight ratio
    |dw| / |w| of that one iteration and per spectrally normalised layer the sigma its forward divides by beside its top singular
    value (`locate_amd.dynamics`), by launches beside the training step; `OUT/error/{epoch}-dynamics.npz` holds an epoch's records;
  * `formats=` / `--formats-every N` (off by default; eager runs only - not with `--graph`): every N-th iteration the operands of
    every dense contraction - gathered activations, output gradients, weights - are audited against five candidate number formats
    (`locate_amd.formats`): what each would flush, push into its subnormals or clamp, and the signal-to-noise ratio left;
    `OUT/error/{epoch}-formats.npz` holds an epoch's records;
  * `--clip-grad-norm X` / `--no-skip-nonfinite` (without either, nothing below happens): both networks are stepped by
    `GuardedNadam` (`locate_amd.guard`) instead of `Nadam`: a step whose gradients hold a NaN or an Inf is skipped on the device
    (unless `--no-skip-nonfinite`), and with X > 0 the gradients are scaled down to the global norm X.  `OUT/error/{epoch}-guard.json`
    holds both optimizers' counters, `OUT/trainer.torch` carries them through `--resume`, and a run whose optimizer has skipped
    `--max-consecutive-skips` steps in a row stops with `GuardExhausted` like a run that holds a NaN does;
  * `snapshot=` / `--rollback-every N` (off by default; needs `--stats-every` or a guarded optimizer, or nothing would ever notice a
    failure): a last-good copy of the whole training state is kept in device memory (`locate_amd.snapshot`), renewed at the
    progress line once N iterations lie behind the last one.  Where the run would stop with `NonFiniteError` or `GuardExhausted`
    it returns to that copy instead and goes on with the next batches - at most `--max-rollbacks` times, recorded in
    `OUT/error/rollbacks.json`; after that it stops as before.  Two more copies of weights and moments in device memory;
  * `spill_every=` / `--spill-every N` (off by default; needs `--rollback-every`): once N iterations lie behind the last one, the
    committed snapshot goes to `OUT/spill/spill-K.bin` in the background (`locate_amd.spill`) - the training stream does not wait -
    and `--resume` continues from that file, bit for bit, when it is newer than the last `trainer.torch`: a killed job loses
    minutes, not the epoch.  One pinned host buffer of a snapshot slot's size;
  * `neighbours=` / `--neighbours IMAGES` (off by default): after every epoch the nearest training images of the sample picture's
    images, exact in the 8-bit domain (`locate_amd.neighbours`): a record in `OUT/error/neighbours.json` and the picture
    `OUT/error/{epoch}-neighbours.png` of rows [sample | its `--neighbours-k` nearest training images].  The evaluation has no side
    effect on the training; the bank is one more copy of the training set's canonical views, as bytes, in device memory;
  * `manifold=` / `--manifold IMAGES` (off by default): after every epoch precision, recall, density and coverage of IMAGES
    generated samples against IMAGES real images (`locate_amd.manifold`, `--manifold-k` neighbours per ball), exact in the 8-bit
    domain, with a real-against-real baseline: a record in `OUT/error/manifold.json`.  It tells lost modes from lost quality.  The
    evaluation has no side effect on the training; under data parallelism only rank 0 evaluates;
  * `spectrum=` / `--spectrum-images N` (off by default): after every epoch the radial power spectrum of N generated samples
    against N real images (`locate_amd.spectrum`, `--spectrum-window hann` for a Hann window), with a real-against-real baseline:
    a record in `OUT/error/spectrum.json`.  It shows the excess at high frequencies and the checkerboard that up-convolutions
    leave.  The evaluation has no side effect on the training; under data parallelism only rank 0 evaluates;
  * `msssim=` / `--msssim-pairs N` (off by default): after every epoch the multi-scale SSIM between N pairs of generated samples
    (`locate_amd.msssim`) beside that of N pairs of real images: a record in `OUT/error/msssim.json`.  It says how alike the samples
    are, scale by scale; with `--ema-half-life` also how alike the live and the averaged generator's images of the same latents are.
    The evaluation has no side effect on the training; under data parallelism only rank 0 evaluates;
  * `modes=` / `--modes SAMPLES` (off by default): after every epoch the Number of statistically Different Bins of SAMPLES generated
    samples (`locate_amd.modes`): `--modes-images` real images are clustered into `--modes-bins` k-means cells, exactly, in the 8-bit
    domain, the samples are assigned to the cells and every cell's share is tested against the real images', with a real-against-
    real baseline: a record in `OUT/error/modes.json` and the picture `OUT/{epoch}-modes.png` of the cells' centres, the most
    under-represented first.  It names the modes that are missing.  The evaluation has no side effect on the training; under
    data parallelism only rank 0 evaluates;
  * `--diffaugment POLICY` (off by default): every batch the discriminator sees passes through the differentiable augmentation of
    `locate_amd.augment`; `--ada-target X` beside it (off by default: the policy at full strength) makes it adaptive - every op is
    applied per image with a probability p that two launches beside the step steer from r_t = E[sign(D(real))] (`--ada-kimg`,
    `--ada-interval`, `--ada-initial-p`, `--ada-p-max`).  The ring of {iteration, r_t, p} is flushed at the progress line, and
    `OUT/error/ada.json` - {"curve": [{"iteration", "r_t", "p"}, ...], "p", "r_t", "updates", "ups", "downs", "nonfinite"}, the
    curve of the whole run, resumes included - is written after every epoch and when `max_iterations` stops the run.
    `OUT/trainer.torch` and the spill's host state carry p, the open window and both random streams under "augment"; a state saved
    with `--ada-target` is refused without it and the other way round.  Not under data parallelism;
  * `--lecam WEIGHT` (off by default): the LeCam regulariser of `locate_amd.lecam` in the D loss - WEIGHT times the mean squared
    distance of D(real) from the moving average of mean D(G(z)) and of D(G(z)) from that of mean D(real), switched on after
    `--lecam-warmup` observed iterations (`--lecam-decay`: the averages' decay; `--lecam-two-sided`: the paper's equation in place
    of the released code's clamped form).  One launch beside the step moves the two averages after every iteration, eager or
    replayed; their ring is flushed at the progress line, and `OUT/error/lecam.json` - {"curve": [{"iteration", "anchor_real",
    "anchor_fake", "mean_real", "mean_fake", "accepted"}, ...], "anchor_real", "anchor_fake", "observations", "accepted",
    "nonfinite", "active"}, the curve of the whole run, resumes included - is written after every epoch and when `max_iterations`
    stops the run.  `--lecam 0` records the curve and leaves the run bit for bit what it is without.  `OUT/trainer.torch` and the
    spill's host state carry the averages under "lecam"; a state saved with other settings is refused, a state without one starts
    the averages at the resumed iteration.  Not under data parallelism;
  * `--topk-floor F` (off by default): top-k training of the generator, `locate_amd.topk` - the G-step's loss and gradient run over
    the k fakes with the highest D(G(z)) only, k = the batch size times `--topk-gamma` to the power of the periods done, never below
    F times the batch size; a period is `--topk-every` iterations (default: one pass over the image store).  k is moved before the
    iteration, eager or replayed; the selection's ring is flushed at the progress line, and `OUT/error/topk.json` - {"curve":
    [{"launch", "k", "active", "threshold", "mean_all", "mean_kept", "nonfinite"}, ...], "k", "k_used", "launches", "nonfinite",
    "active", "threshold", "mean_all", "mean_kept"}, one row per launch of the G-step's loss over the whole run, resumes included -
    is written after every epoch and when `max_iterations` stops the run.  The printed g_error is the loss over the kept k.
    `--topk-gamma 1` leaves the run bit for bit what it is without.  `OUT/trainer.torch` and the spill's host state carry the record
    and the curve under "topk"; a state saved with other settings is refused; a rollback does not rewind it."""
import argparse
import json
import os
import sys
import time
from datetime import timedelta

import torch

from .checkpoint import load_checkpoint, save_checkpoint
from .monitor import LossHistory, Sampler
from .train import TrainLoop

MAIN_N = 2 ** 10          # libs/config.py:67
STATE_FILE = "trainer.torch"
EMA_FILE = "netG_ema.torch"


# ---- the reference's schedule (libs/config.py:19-30, main.py:109-116), per 0-based epoch e ----
def reference_miniter(e, minibatches=8):
    return int((e + 1) * minibatches)


def reference_subepochs(e):
    return (e + 1) ** 2


def reference_print_every(batch, main_n=MAIN_N):
    return max(1, main_n // max(batch, 64))


def reference_image_interval(batch, main_n=MAIN_N):
    return max(1, 16 * main_n // batch)


def picture_name(sub, i, subepochs, batches):
    """`{sub+1:0{sub_len}d}-{i:0{batch_len}d}.png`, or `...-END.png` for i = None (main.py:204-205, 221)."""
    head = "%0*d" % (len(str(subepochs)), sub + 1)
    return head + ("-END.png" if i is None else "-%0*d.png" % (len(str(batches)), i))


def _write_json(path, obj):
    """to a .tmp, then renamed: a reader never sees half a file"""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path + ".tmp", "w") as f:
        json.dump(obj, f)
    os.replace(path + ".tmp", path)
    return path


class Trainer:
    """step: a `TrainStep`; pipeline: an `InputPipeline`; out: the output folder.

    Schedule per epoch e (0-based): `miniter_function(e)` (default (e + 1) * minibatches, minibatches = step.minibatches),
    `subepoch_function(e)` (default (e + 1)^2), `print_every_function(batch)` (default max(1, MAIN_N // max(batch, 64))) and
    `image_interval_function(batch)` (default max(1, 16 * MAIN_N // batch)).  In every sub-pass the batch counter i restarts at 1;
    the print and the sample checks sit inside `if i % miniter == 0`, as in the reference.

    Files: `out/{e+1}/{sub+1}-{i}.png` and `...-END.png` (zero-padded like the reference's), `out/error/{e+1}.json` (and .svg
    where matplotlib imports), the checkpoint files and `out/trainer.torch`.

    graphed=True replays the iteration as hipGraphs (`GraphedTrainStep`).  It is accepted only when miniter == 1 and diters == 1
    in every epoch of the run - so `epochs` must be given - and raises ValueError otherwise.  SIDE EFFECT, as documented on
    `GraphedTrainStep`: building it runs max(warmup, 2) = 2 REAL training iterations eagerly on the run's first batch before
    the capture, so the weights, u / v and Nadam states advance by two steps more than the iteration count says (again after
    every resume).

    sampler_options: passed to `Sampler` (nrow, padding, advance_spectral_norm - True, the reference's behaviour, by default).
    log: a callable taking one line of text (the progress line), or None.

    swd: a `SlicedWasserstein` whose reference is set, or None (the default: nothing below happens).  After each epoch's loss
    curves and before the state is saved, `swd.evaluate(gen)` runs and {"epoch", "iterations", "levels", "mean"} is appended to the
    list in `out/error/swd.json` (a resumed run appends to the list it finds).  The evaluation leaves weights, u / v and
    optimizer states untouched, so the trajectory is that of a run without it.  Under data parallelism only rank 0 should be
    given one, as with the sampler.

    average: an `AveragedGenerator` over step.gen, or None (the default: nothing below happens, and every file, record and key is
    what it is without this argument).  `average.update()` runs after every iteration of this loop, on the stream the iteration
    was issued on: ONE update per trainer iteration - the two warm-up iterations that `GraphedTrainStep` runs when it is built
    (above) belong to the iteration that builds it and are followed by one update, not three.  A second `Sampler` over
    `average.generator` shares the first one's fixed latents and never advances u / v: beside every picture `X.png` it writes
    `X.ema.png`.  The metric is evaluated for both generators; its record gains "average": {"levels", "mean"}.  save_state() also
    writes `netG_ema.torch` - the averaged weights in the reference's `state_dict()` layout, which load into the reference's
    Generator for inference - and puts `average.state_dict()` under "average" in trainer.torch; resume() restores it, so a resumed
    run's average continues the uninterrupted run's bit for bit (eager; a graphed run's two warm-up iterations per resume move
    the weights it follows).  Resuming from a trainer.torch without an average starts it from the resumed weights.  Under data
    parallelism only rank 0 needs one: the weights are equal on every rank.

    stats: a `RunStatistics` over step.gen and step.dis, or None (the default: nothing below happens, and every file, record and key
    is what it is without this argument).  `stats.record(iterations)` follows every `stats_every`-th iteration of this loop
    (counted across resumes; 0: only the records below), after `average.update()` and on the same stream: it reads the post-step
    weights and the gradients the optimizer steps consumed, and writes nothing the training reads.  `stats.check()` runs where
    this loop reads from the device anyway - with the progress line - and IMMEDIATELY BEFORE every save_state(), at the end of
    an epoch and when `max_iterations` stops the run; if the last iteration has no record, one is taken first, so no state is
    saved unchecked.  On `NonFiniteError` the trainer writes `out/error/nonfinite.json` - {"iteration", "epoch" (1-based),
    "tensors": [[name, count], ...]} - does NOT save the state, so the files of the last good save stay byte for byte, and
    re-raises.  `out/error/{e+1}-stats.npz` (`RunStatistics.save`) is written beside the loss curves and holds the records of that
    epoch taken by this call of run(); the records start empty in every epoch, like the curves.  Under data parallelism only
    rank 0 needs one: the weights, and the gradients after the exchange, are equal on every rank.

    dynamics: a `RunDynamics` over step.gen and step.dis, or None (the default: nothing below happens, and every file, record and
    key is what it is without this argument); `dynamics_every`: N >= 0, 0 (the default) is off.  `dynamics.mark()` is issued before
    the iteration that makes `iterations` a multiple of N and `dynamics.record(iterations)` after it - behind `average.update()`
    and the statistics' record, on the same stream - so a record's delta is exactly what that one iteration (its D step and its G
    step) did to the weights, and the cost falls on every N-th iteration only.  Both only read what the training owns.
    `out/error/{e+1}-dynamics.npz` (`RunDynamics.save`) is written beside `{e+1}-stats.npz` and holds the records of that epoch
    taken by this call of run(); the records start empty in every epoch.  Nothing goes into trainer.torch: after a resume the top
    singular vectors start again from the live u / v and the file holds the records since the resume, as with the statistics.
    An iteration that does not step a network's optimizer (miniter > 1: the generator is stepped every miniter-th iteration) shows
    `unchanged == n` for that network's weights.  After a rollback the next record is simply taken on the restored weights.  With
    graphed=True the iteration that builds the graphs runs its two warm-up iterations too: a record around it spans all three.
    Under data parallelism only rank 0 needs one.

    formats: a `FormatAudit` over step.gen and step.dis, or None (the default: nothing below happens, and every file, record and
    key is what it is without this argument); `formats_every`: N >= 0, 0 (the default) is off.  The iteration that makes
    `iterations` a multiple of N runs inside `formats.iteration(iterations)`: the operands of its dense contractions are audited
    against the candidate number formats (`locate_amd.formats`) by launches that only read them, and the cost falls on that
    iteration only.  `out/error/{e+1}-formats.npz` (`FormatAudit.save`) is written beside `{e+1}-dynamics.npz` and holds the
    records of that epoch taken by this call of run().  Nothing goes into trainer.torch.  A replayed graph runs no Python, so
    graphed=True with formats_every > 0 raises ValueError.  Under data parallelism only rank 0 needs one.

    Guarded optimizers: where step.gen_opt or step.dis_opt is a `GuardedNadam` (anything with `counters()`; with plain `Nadam`s
    nothing below happens, and every file, record and key is what it is today), its counters are read where this loop reads from
    the device anyway - with the progress line - and before every save_state().  An optimizer whose `consecutive_skips` has reached
    `max_consecutive_skips` (default 16, the reference's progress interval at batch 64) would skip every further step too - its
    gradients are non-finite whatever the batch, usually because a weight is: the trainer writes `out/error/nonfinite.json` -
    {"iteration", "epoch", "tensors": [], "guard": {"network", "counters"}} - does NOT save the state and raises
    `GuardExhausted(.iteration, .network)`.  Once per epoch `out/error/{e+1}-guard.json` - {"G": counters, "D": counters}, the
    guarded ones only - is written beside the loss curves; save_state() puts the counters under "guard" in trainer.torch and
    resume() restores them.

    snapshot: a `TrainingSnapshot` over `step` (and `average`), or None (the default: nothing below happens, and every file, record
    and key is what it is without this argument).  It needs `stats` or a guarded optimizer - nothing else ever notices a failure -
    and raises ValueError without.  `snapshot.take(iterations)` follows the checks of a progress line once they have passed and at
    least `rollback_every` iterations lie behind the last take (or the start of the run): two launches on the same stream, no host
    read; the take commits itself on the device only if every word it copied is finite.  Where the checks above would stop the run
    - at the progress line and before each save - the trainer instead calls `snapshot.restore()`, while the rollbacks so far
    (counted across resumes) are fewer than `max_rollbacks` and a committed snapshot exists, appends {"iteration", "to_iteration",
    "epoch", "cause": "nonfinite" | "guard", "tensors" or "guard"} to the list in `out/error/rollbacks.json` and goes on with the
    NEXT batches: the pipeline, the latent stream, i, `iterations`, the loss history and the statistics records are not rewound,
    and the bad record stays in `{e+1}-stats.npz` as evidence.  Before a save the restored state is recorded and checked like any
    other, then saved.  `nonfinite.json` is written only when the run does stop.  trainer.torch gains "rollbacks"; a resumed run
    starts with no committed slot.  Limits: a state that is finite but already diverging can be committed - the run then fails
    again after the rollback and stops once `max_rollbacks` is used up; data parallelism is out of scope (`TrainingSnapshot`).

    spill_every: 0 (the default: nothing below happens, and every file, record and key is what it is without this argument) or N > 0,
    which needs `snapshot` and raises ValueError without.  The trainer makes a `SnapshotSpill(snapshot, out/spill)`.  At a progress
    line, after the checks have passed and BEFORE the take that follows them, `spill.begin()` runs once at least N iterations lie
    behind the last spill begun: what goes to disk is the slot committed at an EARLIER progress line - finite at its take, and the
    run has passed its checks again since.  The take itself goes through `spill.take`, whose host state is what save_state() puts
    into trainer.torch and netG.extra.torch, as of that take: epoch, sub, i, iterations, the pipeline's, the latent generator's
    and the loss history's state, the fixed latents, the average's `updates` and `one_minus_beta`, the guards' counters,
    `rollbacks`, `gen.noise` (constant: copied to the host once, at construction) and the `dis_uv_trainable` flag.  resume() compares
    `SnapshotSpill.latest(out/spill)` with trainer.torch - which may then be missing - and continues from the one with more
    `iterations`: from a spill through `restore_training_state`, with the host state restored exactly as trainer.torch's is; the
    choice goes into `out/error/resumes.json` as {"from": "spill" | "save", "iterations"}.  run() calls `spill.wait()` before it
    returns or re-raises, so a run that ends normally leaves no half-started writer.  Out of scope: data parallelism, compression,
    an asynchronous save_state(), bit-exact graphed resumes (two warm-up iterations per resume, as today).

    neighbours: a `NearestNeighbours` whose reference is set, or None (the default: nothing below happens, and every file, record and
    key is what it is without this argument).  After each epoch's SWD record, `neighbours.evaluate(gen, latents=sampler.fixed_noise)`
    runs - the samples are the ones of the sample picture - and {"epoch", "iterations", "images", "k", "generated_to_real",
    "generated_to_generated", "real_to_real", "real_among_themselves", "nonfinite", "index"} is appended to the list in
    `out/error/neighbours.json` (a resumed run appends to the list it finds); `out/error/{e+1}-neighbours.png` shows every sample beside
    its nearest training images.  With `average`, the same keys for the averaged generator go under "average" and its picture to
    `{e+1}-neighbours.ema.png`.  The evaluation leaves weights, u / v and optimizer states untouched.  Under data parallelism only
    rank 0 should be given one.

    manifold, spectrum, msssim, modes: a `ManifoldMetrics` and a `RadialSpectrum` whose reference is set, a `MultiScaleSSIM` (with its
    "real" reference, if wanted) and a `BinnedModes` whose reference is set, or None each (the default: nothing below happens, and every file, record
    and key is what it is without that argument).  After each epoch's neighbours record, in this order, the metric's `evaluate(gen)`
    runs on the metric's own fixed latents and the record, with "epoch" and "iterations", is appended to the list in
    `out/error/manifold.json`, `spectrum.json`, `msssim.json` and `modes.json` (written to a .tmp and renamed; a resumed run appends to
    the list it finds).  With `average`, the averaged generator's record - without the baseline (msssim: without "real"), which is the
    same - goes under "average", and for msssim `msssim.evaluate_against(gen, average.generator)`, the two generators' images of the
    same latents against each other, under "average_to_live".  For modes, `out/{e+1}-modes.png` shows the bins' centres in the live
    record's order, the most under-represented first.  The evaluations leave weights, u / v and optimizer states untouched.  Under
    data parallelism only rank 0 should be given them.

    All six records go through `_append_record`, the one place that reads, appends to and writes a list in `out/error`."""

    def __init__(self, step, pipeline, out, epochs=None, max_iterations=None, images=64, seed=999, diters=1, minibatches=None,
                 mean_window=16, graphed=False, fixed_noise=None, miniter_function=None, subepoch_function=None,
                 print_every_function=None, image_interval_function=None, sampler_options=None, log=None, swd=None,
                 average=None, stats=None, stats_every=16, max_consecutive_skips=16, snapshot=None, rollback_every=256,
                 max_rollbacks=3, spill_every=0, dynamics=None, dynamics_every=0, neighbours=None, manifold=None,
                 formats=None, formats_every=0, spectrum=None, msssim=None, modes=None):
        self.step, self.pipeline, self.out = step, pipeline, str(out)
        self.gen, self.dis = step.gen, step.dis
        self.augment = getattr(step, "augment", None)          # a DiffAugment: its rows are drawn before every iteration
        self.adaptive = hasattr(self.augment, "observe")          # an AdaptiveDiffAugment: observed after every iteration
        self.lecam = getattr(step, "lecam", None)          # a LeCam regulariser: observed after every iteration (TrainLoop does, eagerly)
        self.topk = getattr(step, "topk", None)          # a TopK selection: k is moved before every iteration (TrainLoop does, eagerly)
        self.batch = pipeline.batch
        self.epochs = None if epochs is None else int(epochs)
        self.max_iterations = None if max_iterations is None else int(max_iterations)
        m = step.minibatches if minibatches is None else int(minibatches)
        self.miniter_function = miniter_function or (lambda e: reference_miniter(e, m))
        self.subepoch_function = subepoch_function or reference_subepochs
        self.print_every = (print_every_function or reference_print_every)(self.batch)
        self.image_interval = (image_interval_function or reference_image_interval)(self.batch)
        if self.print_every < 1 or self.image_interval < 1:
            raise ValueError("print_every and image_interval must be >= 1")
        self.diters = int(diters)
        self.graphed = bool(graphed)
        if self.graphed:
            if self.epochs is None:
                raise ValueError("graphed=True needs `epochs`: the whole schedule must be known to be miniter == 1")
            bad = [e for e in range(self.epochs) if self.miniter_function(e) != 1]
            if bad or self.diters != 1:
                raise ValueError("graphed=True replays whole iterations: miniter == 1 and diters == 1 throughout "
                                 "(miniter is %d in epoch %d, diters %d)" % (self.miniter_function(bad[0]) if bad else 1,
                                                                            bad[0] + 1 if bad else 1, self.diters))
        self.loop = TrainLoop(step, 1, self.diters)          # refuses an adaptive augment beside a data-parallel reducer
        self.device = next(self.gen.parameters()).device
        self._sampler_args = dict(fixed_noise=fixed_noise, images=images, seed=seed, **(sampler_options or {}))
        self._sampler = None
        self.history = LossHistory(mean_window)
        self._seed = int(seed)
        self._latent_rng = None
        self.log = log
        self.swd = swd
        self.neighbours = neighbours
        self.manifold = manifold
        self.spectrum = spectrum
        self.msssim = msssim
        self.modes = modes
        self.average = average
        self._ema_sampler = None
        if int(stats_every) < 0:
            raise ValueError("stats_every must be >= 0, got %r" % (stats_every,))
        self.stats, self.stats_every = stats, int(stats_every)
        if int(dynamics_every) < 0:
            raise ValueError("dynamics_every must be >= 0, got %r" % (dynamics_every,))
        self.dynamics, self.dynamics_every = dynamics, int(dynamics_every)
        if int(formats_every) < 0:
            raise ValueError("formats_every must be >= 0, got %r" % (formats_every,))
        if self.graphed and int(formats_every) > 0:
            raise ValueError("graphed=True with formats_every > 0: a replayed graph runs no Python, so the audit's tap sees no "
                             "contraction; audit an eager run")
        self.formats, self.formats_every = formats, int(formats_every)
        if int(max_consecutive_skips) < 1:
            raise ValueError("max_consecutive_skips must be >= 1, got %r" % (max_consecutive_skips,))
        self.max_consecutive_skips = int(max_consecutive_skips)
        if int(rollback_every) < 1 or int(max_rollbacks) < 0:
            raise ValueError("rollback_every must be >= 1 and max_rollbacks >= 0, got %r and %r" % (rollback_every, max_rollbacks))
        self.snapshot, self.rollback_every, self.max_rollbacks = snapshot, int(rollback_every), int(max_rollbacks)
        if snapshot is not None and stats is None and not self._guards():
            raise ValueError("a snapshot needs `stats` or a guarded optimizer: nothing else would ever trigger a rollback")
        if int(spill_every) < 0:
            raise ValueError("spill_every must be >= 0, got %r" % (spill_every,))
        self.spill_every = int(spill_every)
        if self.spill_every and snapshot is None:
            raise ValueError("spill_every needs a snapshot: what goes to disk is its committed slot")
        self.spill = None
        if self.spill_every:
            from .spill import SnapshotSpill
            self.spill = SnapshotSpill(snapshot, os.path.join(self.out, "spill"))
            self._noise_host = self.gen.noise.detach().to("cpu").clone()          # constant during training
            self._fixed_noise_host = None
        self._last_spill = 0          # `iterations` at the last spill begun
        self.rollbacks = 0          # counted across resumes
        self._last_take = 0          # `iterations` at the last take (at the start of the run, before the first)
        self._unrecorded = False          # a restored state that the statistics have not seen yet
        self.epoch, self.sub, self.i, self.iterations = 0, 0, 0, 0
        self._runner = None
        self.written = []

    # ---- device-side helpers, made on first use (the schedule can be inspected without a GPU) ------------------
    @property
    def sampler(self):
        if self._sampler is None:
            self._sampler = Sampler(self.gen, **self._sampler_args)
        return self._sampler

    @property
    def ema_sampler(self):
        """the averaged generator's sampler: the first one's latents (the same tensor), u / v never advanced"""
        if self._ema_sampler is None:
            options = {k: v for k, v in self._sampler_args.items() if k in ("nrow", "padding")}
            self._ema_sampler = Sampler(self.average.generator, fixed_noise=self.sampler.fixed_noise, advance_spectral_norm=False, **options)
        return self._ema_sampler

    @property
    def _latent_gen(self):
        if self._latent_rng is None:
            self._latent_rng = torch.Generator(device=self.device)
            self._latent_rng.manual_seed(self._seed + 1)
        return self._latent_rng

    # ---- schedule -------------------------------------------------------------------------------------------
    def schedule(self, e):
        """{miniter, subepochs, print_every, image_interval} of 0-based epoch e"""
        return {"miniter": int(self.miniter_function(e)), "subepochs": int(self.subepoch_function(e)),
                "print_every": self.print_every, "image_interval": self.image_interval}

    def picture_path(self, e, sub, i):
        return os.path.join(self.out, str(e + 1), picture_name(sub, i, int(self.subepoch_function(e)), self.pipeline.batches_per_epoch))

    # ---- state ----------------------------------------------------------------------------------------------
    def save_state(self):
        """The checkpoint files and trainer.torch (written last: it names a state the other files already hold)."""
        files = save_checkpoint(self.out, self.gen, self.dis, self.step.gen_opt, self.step.dis_opt)
        state = {"epoch": self.epoch, "sub": self.sub, "i": self.i, "iterations": self.iterations,
                 "pipeline": self.pipeline.state_dict(), "fixed_noise": self.sampler.fixed_noise.detach().cpu(),
                 "latent_state": self._latent_gen.get_state(), "history": self.history.state_dict()}
        if self.average is not None:
            ema = os.path.join(self.out, EMA_FILE)
            torch.save(self.average.generator_state_dict(), ema + ".tmp")
            os.replace(ema + ".tmp", ema)
            files.append(ema)
            state["average"] = self.average.state_dict()
        if self._guards():
            state["guard"] = {tag: opt.counters_state() for tag, opt in self._guards()}
        if self.snapshot is not None:
            state["rollbacks"] = int(self.rollbacks)
        if self.augment is not None:
            state["augment"] = self.augment.state_dict()
        if self.lecam is not None:
            state["lecam"] = self.lecam.state_dict()
        if self.topk is not None:
            state["topk"] = self.topk.state_dict()
        path = os.path.join(self.out, STATE_FILE)
        torch.save(state, path + ".tmp")
        os.replace(path + ".tmp", path)
        return files + [path]

    def resume(self):
        """Continue from what save_state() left in `out` - or, with a spill, from the newer of that and the last valid spill file."""
        path = os.path.join(self.out, STATE_FILE)
        found = None
        if self.spill is not None:
            from .spill import SnapshotSpill, restore_training_state
            found = SnapshotSpill.latest(self.spill.folder)
        if found is None or os.path.exists(path):
            state = torch.load(path, map_location="cpu", weights_only=True)
            if found is not None and int(found.host_state["iterations"]) <= int(state["iterations"]):
                found = None
        if found is not None:
            restore_training_state(found, self.step, self.average)
            state = found.host_state
        else:
            load_checkpoint(self.out, self.gen, self.dis, self.step.gen_opt, self.step.dis_opt)
        if self.spill is not None:
            _write_json(os.path.join(self.out, "error", "resumes.json"),
                        {"from": "spill" if found is not None else "save", "iterations": int(state["iterations"])})
        self.epoch, self.sub, self.i, self.iterations = (int(state[k]) for k in ("epoch", "sub", "i", "iterations"))
        self.pipeline.load_state_dict(state["pipeline"])
        noise = state["fixed_noise"]
        if tuple(noise.shape) != tuple(self.sampler.fixed_noise.shape):
            raise ValueError("trainer.torch holds fixed latents of shape %s, this run's are %s" % (tuple(noise.shape), tuple(self.sampler.fixed_noise.shape)))
        self.sampler.fixed_noise.copy_(noise)
        self._latent_gen.set_state(state["latent_state"])
        self.history.load_state_dict(state["history"])
        if self.average is not None and found is None:          # a spill's average went in with its tensors
            if "average" in state:
                self.average.load_state_dict(state["average"])
            else:
                self.average.reset()          # a run that had none: the average starts from the resumed weights
        for tag, opt in self._guards():
            if tag in state.get("guard", {}):
                opt.load_counters_state(state["guard"][tag])
        if self.snapshot is not None:
            self.rollbacks = int(state.get("rollbacks", 0))
        if self.augment is not None and "augment" in state:          # a run that had none: the parameter stream starts here
            self.augment.load_state_dict(state["augment"])
        if self.lecam is not None and "lecam" in state:          # a run that had none: the anchors start here
            self.lecam.load_state_dict(state["lecam"])
        if self.topk is not None and "topk" in state:          # a run that had none: the curve starts here, k follows the iteration count
            self.topk.load_state_dict(state["topk"])
        self._last_take = self.iterations         # no committed slot yet: the first take is rollback_every iterations away
        self._last_spill = self.iterations
        return self

    def _spill_host_state(self):
        """what save_state() puts into trainer.torch and netG.extra.torch, as of now: the host state of a take that may be spilled"""
        if self._fixed_noise_host is None:
            self._fixed_noise_host = self.sampler.fixed_noise.detach().cpu()          # constant during a run
        uv = [p.requires_grad for n, p in self.dis.named_parameters() if n.endswith(("weight_u", "weight_v"))]
        state = {"epoch": self.epoch, "sub": self.sub, "i": self.i, "iterations": self.iterations,
                 "pipeline": self.pipeline.state_dict(), "fixed_noise": self._fixed_noise_host,
                 "latent_state": self._latent_gen.get_state(), "history": self.history.state_dict(),
                 "rollbacks": int(self.rollbacks), "noise": self._noise_host, "dis_uv_trainable": bool(uv) and all(uv)}
        if self.average is not None:
            state["average"] = {"updates": int(self.average.updates), "one_minus_beta": float(self.average.one_minus_beta)}
        if self._guards():
            state["guard"] = {tag: opt.counters_state() for tag, opt in self._guards()}
        if self.augment is not None:
            state["augment"] = self.augment.state_dict()
        if self.lecam is not None:
            state["lecam"] = self.lecam.state_dict()
        if self.topk is not None:
            state["topk"] = self.topk.state_dict()
        return state

    def _guards(self):
        """[("G" | "D", optimizer)] of the optimizers that keep guard counters"""
        return [(tag, opt) for tag, opt in (("G", self.step.gen_opt), ("D", self.step.dis_opt)) if hasattr(opt, "counters")]

    def _check_guards(self):
        """One small device read per guarded optimizer; {"G": counters, "D": counters}.  An optimizer that has skipped
        max_consecutive_skips steps in a row leaves out/error/nonfinite.json and raises."""
        from .guard import GuardExhausted
        seen = {tag: opt.counters() for tag, opt in self._guards()}
        for tag, c in seen.items():
            if c["consecutive_skips"] >= self.max_consecutive_skips:
                guard = {"network": tag, "counters": c}
                if self._rollback({"iteration": self.iterations, "cause": "guard", "guard": guard}):
                    return {tag: opt.counters() for tag, opt in self._guards()}          # consecutive_skips restarted at 0
                self._write_nonfinite({"iteration": self.iterations, "epoch": self.epoch + 1, "tensors": [], "guard": guard})
                raise GuardExhausted(self.iterations, tag, c["consecutive_skips"])
        return seen

    def _save_guards(self, epoch):
        return _write_json(os.path.join(self.out, "error", "%d-guard.json" % epoch), self._check_guards())

    def _write_nonfinite(self, record):
        self.written.append(_write_json(os.path.join(self.out, "error", "nonfinite.json"), record))

    def _check_stats(self, before_save=False):
        """stats.check(); before a save, preceded by a record of the state that is about to be saved if it has none.  A run that
        holds a non-finite value leaves out/error/nonfinite.json and raises."""
        from .stats import NonFiniteError
        while True:
            if before_save and self.iterations > 0 and (self.stats.last_iteration != self.iterations or self._unrecorded):
                self._record_stats()
            try:
                self.stats.check()
                return
            except NonFiniteError as err:
                tensors = [list(t) for t in err.tensors]
                if not self._rollback({"iteration": err.iteration, "cause": "nonfinite", "tensors": tensors}):
                    self._write_nonfinite({"iteration": err.iteration, "epoch": self.epoch + 1, "tensors": tensors})
                    raise
            if not before_save:
                return          # rolled back: the run goes on; before a save the restored state is recorded and checked too

    def _record_stats(self):
        self.stats.record(self.iterations)          # two launches on this stream, no host read
        self._unrecorded = False

    def _checks(self, before_save=False):
        """The statistics' and the guards' checks, where the loop reads from the device anyway and before every save."""
        if self.stats is not None:
            self._check_stats(before_save)
        if self._guards():
            self._check_guards()
            if before_save and self.stats is not None and self._unrecorded:          # the guard rolled the run back just now
                self._check_stats(before_save)

    def _rollback(self, record):
        """Back to the last good snapshot instead of stopping: True when the run now holds that state (one more record in
        out/error/rollbacks.json), False when it has to stop as it would without a snapshot."""
        if self.snapshot is None or self.rollbacks >= self.max_rollbacks:
            return False
        from .snapshot import NoSnapshot
        try:
            to_iteration = self.snapshot.restore()
        except NoSnapshot:
            return False
        self.rollbacks += 1
        self._unrecorded = True
        path = os.path.join(self.out, "error", "rollbacks.json")
        records = []
        if os.path.exists(path):
            with open(path) as f:
                records = json.load(f)
        head = {"iteration": record.pop("iteration"), "to_iteration": int(to_iteration), "epoch": self.epoch + 1}
        records.append(dict(head, **record))
        path = _write_json(path, records)
        if path not in self.written:
            self.written.append(path)
        return True

    # ---- the loop -------------------------------------------------------------------------------------------
    def _iteration(self):
        latent_shape = (self.batch, self.gen.g_in)
        if not self.graphed:
            latent = torch.randn(latent_shape, device=self.device, generator=self._latent_gen)          # main.py:142
            real, aug = self.pipeline.next_batch()
            self.loop.iterations = self.iterations          # what the top-k schedule counts: i restarts with every sub-pass
            return self.loop.iteration(latent, real, aug)          # draws the augmentation's rows and moves k itself
        if self.augment is not None:
            self.augment.draw()          # the graphs read the rows at a fixed address: whatever was uploaded last
        if self.topk is not None:
            self.topk.advance(self.iterations)          # likewise word 0 of its record: the capture's warm-up runs with this k too
        if self._runner is None:
            from .graph import GraphedTrainStep
            latent = torch.randn(latent_shape, device=self.device, generator=self._latent_gen)
            real, aug = self.pipeline.next_batch()
            self._runner = GraphedTrainStep(self.step, latent, real, aug)          # runs two real iterations on this batch
        else:
            lat, real, aug = self._runner.inputs
            lat.copy_(torch.randn(latent_shape, device=self.device, generator=self._latent_gen))
            self.pipeline.next_batch(out_real=real, out_aug=aug)          # written straight into the graphs' static inputs
        out = self._runner.replay()
        if self.adaptive:
            self.augment.observe(out["d_true"])          # the replay's logits; the capture's two warm-up iterations are not observed
        if self.lecam is not None:
            self.lecam.observe(out["d_true"], out["d_gen"])          # likewise: the anchors move between two replays
        return out

    def _progress(self, e, sub, i, first, subepochs, batches, started):
        """first: the position this call of run() entered the sub-pass at (not 0 after a resume): the rate counts from there"""
        pairs = self.history.flush()          # the one host read of the losses
        if self.adaptive:
            self.augment.flush()          # the ring's new {iteration, r_t, p} rows, here where the loop reads from the device anyway
        if self.lecam is not None:
            self.lecam.flush()          # the anchors' curve likewise
        if self.topk is not None:
            self.topk.flush()          # and the selection's rows
        before = self.rollbacks
        self._checks()
        if self.spill is not None and self.rollbacks == before and self.iterations - self._last_spill >= self.spill_every:
            if self.spill.begin():          # the slot committed at an earlier progress line; this stream only records an event
                self._last_spill = self.iterations
        if self.snapshot is not None and self.rollbacks == before and self.iterations - self._last_take >= self.rollback_every:
            # two launches on this stream, no host read; commits itself if finite.  With a spill the take's host state goes with it:
            # host values, and the guards' counters read once more (64 bytes each, at a line that reads from the device anyway)
            if self.spill is not None:
                self.spill.take(self.iterations, self._spill_host_state())
            else:
                self.snapshot.take(self.iterations)
            self._last_take = self.iterations
        if self.log is None or not (self.history.d and self.history.g):
            return
        rate = (i - first) / max(time.time() - started, 1e-9)
        eta = str(timedelta(seconds=int((batches - i) / rate)))
        d, g = (pairs[-1] if pairs else (self.history.d[-1], self.history.g[-1]))
        self.log("[%d][%d/%d][%*d/%d] | Rate: %.2f Img/s - %.2f Upd/s | D:%9.4f - G:%9.4f| ETA: %s"
                 % (e + 1, sub + 1, subepochs, len(str(batches)), i, batches, rate * self.batch, rate, d, g, eta))

    def _picture(self, e, sub, i):
        path = self.picture_path(e, sub, i)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        self.written.append(self.sampler.save(path))
        if self.average is not None:
            self.written.append(self.ema_sampler.save(path[:-len(".png")] + ".ema.png"))

    def _append_record(self, name, e, evaluate, keys=None, drop=None, also=None):
        """One record into the list in out/error/NAME.json (a resumed run appends to the list it finds; written to a .tmp and
        renamed): "epoch", "iterations" and what evaluate(gen) returns - `keys` of it, if given.  With an average, the same of
        evaluate(average.generator) without the key `drop` goes under "average", and what also() returns beside it.  Returns the
        file written and the live generator's value."""
        value = evaluate(self.gen)
        path = os.path.join(self.out, "error", name + ".json")
        records = []
        if os.path.exists(path):
            with open(path) as f:
                records = json.load(f)
        records.append(dict({"epoch": e + 1, "iterations": self.iterations}, **{k: value[k] for k in keys or value}))
        if self.average is not None:
            average = evaluate(self.average.generator)
            records[-1]["average"] = {k: average[k] for k in keys or average if k != drop}
            if also is not None:
                records[-1].update(also())
        return _write_json(path, records), value

    def _save_ada(self):
        """out/error/ada.json: the adaptive augmentation's whole curve so far, {"iteration", "r_t", "p"} per closed window (counted
        across resumes), and the counters of this moment"""
        self.augment.flush()
        return _write_json(os.path.join(self.out, "error", "ada.json"), dict(self.augment.status(), curve=self.augment.curve()))

    def _save_lecam(self):
        """out/error/lecam.json: the LeCam regulariser's anchors of this moment and their whole curve so far, one row per observed
        iteration (counted across resumes)"""
        self.lecam.flush()
        return _write_json(os.path.join(self.out, "error", "lecam.json"), dict(self.lecam.status(), curve=self.lecam.curve()))

    def _save_topk(self):
        """out/error/topk.json: the top-k selection's record of this moment and its whole curve so far, one row per launch of the
        G-step's loss (counted across resumes)"""
        self.topk.flush()
        return _write_json(os.path.join(self.out, "error", "topk.json"), dict(self.topk.status(), curve=self.topk.curve()))

    def _measure(self, e):
        """One record of the sliced Wasserstein distance into out/error/swd.json (written to a .tmp and renamed)."""
        return self._append_record("swd", e, self.swd.evaluate, keys=("levels", "mean"))[0]

    def _nearest(self, e):
        """One record of the samples' nearest training images into out/error/neighbours.json (written to a .tmp and renamed) and
        the picture out/error/{e+1}-neighbours.png, for the sampler's fixed latents; returns the files written."""
        keys = ("images", "k", "generated_to_real", "generated_to_generated", "real_to_real", "real_among_themselves", "nonfinite", "index")
        latents, written = self.sampler.fixed_noise, []

        def evaluate(gen):          # the record, then the picture, of one generator
            value = self.neighbours.evaluate(gen, latents=latents)
            name = "%d-neighbours%s.png" % (e + 1, "" if gen is self.gen else ".ema")
            written.append(self.neighbours.save_picture(os.path.join(self.out, "error", name), gen, latents=latents))
            return value
        return [self._append_record("neighbours", e, evaluate, keys=keys)[0]] + written

    def _manifold(self, e):
        """One record of precision / recall / density / coverage into out/error/manifold.json (written to a .tmp and renamed), for
        the metric's own fixed latents; returns the file written."""
        return self._append_record("manifold", e, self.manifold.evaluate, drop="baseline")[0]

    def _spectrum(self, e):
        """One record of the radial power spectrum into out/error/spectrum.json (written to a .tmp and renamed), for the metric's
        own fixed latents; returns the file written."""
        return self._append_record("spectrum", e, self.spectrum.evaluate, drop="baseline")[0]

    def _msssim(self, e):
        """One record of the multi-scale SSIM into out/error/msssim.json (written to a .tmp and renamed), for the metric's own fixed
        latents; returns the file written."""
        return self._append_record("msssim", e, self.msssim.evaluate, drop="real", also=lambda: {
            "average_to_live": self.msssim.evaluate_against(self.gen, self.average.generator)})[0]

    def _modes(self, e):
        """One record of the binned mode coverage into out/error/modes.json (written to a .tmp and renamed), for the metric's own
        fixed latents, and the picture of the bins' centres; returns the files written."""
        path, value = self._append_record("modes", e, self.modes.evaluate, drop="baseline")
        return [path, self.modes.save_picture(os.path.join(self.out, "%d-modes.png" % (e + 1)), value)]

    def run(self):
        """Runs until `epochs` epochs are done or `max_iterations` iterations have been run in all (counted across resumes);
        returns the number of iterations run so far.  State is saved after every epoch and when max_iterations stops the run."""
        try:
            return self._run()
        finally:
            if self.spill is not None:
                self.spill.wait()          # no half-started writer is left behind, whether the run returns or raises

    def _run(self):
        batches = self.pipeline.batches_per_epoch
        while self.epochs is None or self.epoch < self.epochs:
            e = self.epoch
            sched = self.schedule(e)
            miniter, subepochs = sched["miniter"], sched["subepochs"]
            self.loop.miniter = miniter
            while self.sub < subepochs:
                started, first = time.time(), self.i
                self.loop.i = self.i          # i restarts at 1 in every sub-pass (main.py:140)
                while self.i < batches:
                    if self.max_iterations is not None and self.iterations >= self.max_iterations:
                        self._checks(before_save=True)
                        if self.adaptive:
                            self.written.append(self._save_ada())
                        if self.lecam is not None:
                            self.written.append(self._save_lecam())
                        if self.topk is not None:
                            self.written.append(self._save_topk())
                        self.written += self.save_state()
                        return self.iterations
                    followed = self.dynamics is not None and self.dynamics_every and (self.iterations + 1) % self.dynamics_every == 0
                    if followed:
                        self.dynamics.mark()          # one launch on this stream: the base this iteration's delta is taken from
                    if self.formats is not None and self.formats_every and (self.iterations + 1) % self.formats_every == 0:
                        with self.formats.iteration(self.iterations + 1):          # the tap is on for this iteration only
                            out = self._iteration()
                    else:
                        out = self._iteration()
                    if self.average is not None:
                        self.average.update()          # one launch on this stream, behind the iteration's last write
                    self.i += 1
                    self.iterations += 1
                    if self.stats is not None and self.stats_every and self.iterations % self.stats_every == 0:
                        self._record_stats()
                    if followed:
                        self.dynamics.record(self.iterations)          # no host read
                    i = self.i
                    if i % miniter == 0:          # main.py:158
                        self.history.record(out)
                        if i % sched["print_every"] == 0:          # :174
                            self._progress(e, self.sub, i, first, subepochs, batches, started)
                        if i % sched["image_interval"] == 0:          # :194
                            self._picture(e, self.sub, i)
                self._picture(e, self.sub, None)          # :213-225
                self.sub, self.i = self.sub + 1, 0
            if self.stats is not None:
                self._check_stats(before_save=True)          # the epoch's last record, in front of the files that hold it
            self.written += self.history.save(os.path.join(self.out, "error"), e + 1)          # :226-234
            self.history = LossHistory(self.history.mean_window)          # dhist / ghist start empty in every epoch (:107-108)
            if self.stats is not None:
                self.written += self.stats.save(os.path.join(self.out, "error"), e + 1)
                self.stats.clear()
            if self.dynamics is not None and self.dynamics_every:
                self.written += self.dynamics.save(os.path.join(self.out, "error"), e + 1)
                self.dynamics.clear()
            if self.formats is not None and self.formats_every:
                self.written += self.formats.save(os.path.join(self.out, "error"), e + 1)
                self.formats.clear()
            if self._guards():
                self.written.append(self._save_guards(e + 1))         # raises, before the save below, if a guard is exhausted
            if self.adaptive:
                self.written.append(self._save_ada())
            if self.lecam is not None:
                self.written.append(self._save_lecam())
            if self.topk is not None:
                self.written.append(self._save_topk())
            if self.swd is not None:
                self.written.append(self._measure(e))
            if self.neighbours is not None:
                self.written += self._nearest(e)
            if self.manifold is not None:
                self.written.append(self._manifold(e))
            if self.spectrum is not None:
                self.written.append(self._spectrum(e))
            if self.msssim is not None:
                self.written.append(self._msssim(e))
            if self.modes is not None:
                self.written += self._modes(e)
            self.epoch, self.sub = e + 1, 0
            if self.stats is not None:
                self._check_stats(before_save=True)
            self.written += self.save_state()          # :235-236
        return self.iterations


def parser():
    """The command line's argument parser (needs no GPU)."""
    ap = argparse.ArgumentParser(prog="python -m locate_amd.run", description="Train on a prepared image store and watch the run.")
    ap.add_argument("--store", required=True, help="uint8 [N, H, W, 3] .npy file (locate_amd.data.prepare_folder)")
    ap.add_argument("--image-size", type=int, required=True)
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--epochs", type=int, default=None, help="default: until interrupted, like the reference")
    ap.add_argument("--max-iterations", type=int, default=None, help="stop (and save) after this many iterations in all")
    ap.add_argument("--images", type=int, default=64, help="images in the sample picture")
    ap.add_argument("--seed", type=int, default=999)
    ap.add_argument("--minibatches", type=int, default=8, help="MINIBATCHES of the reference; 1 gives miniter = 1 in the first epoch")
    ap.add_argument("--diters", type=int, default=1)
    ap.add_argument("--graph", action="store_true", help="replay the iteration as hipGraphs (needs miniter = diters = 1 throughout)")
    ap.add_argument("--resume", action="store_true", help="continue from the files in --out")
    ap.add_argument("--keep-spectral-norm", action="store_true",
                    help="sampling leaves the generator's u / v untouched (the reference's sampling pass advances them)")
    ap.add_argument("--swd-images", type=int, default=0,
                    help="after every epoch, the sliced Wasserstein distance of the generator against this many real images "
                         "(OUT/error/swd.json); 0: off")
    ap.add_argument("--ema-half-life", type=float, default=0.0, metavar="IMAGES",
                    help="keep an exponential moving average of the generator's weights whose weight of an old value halves every "
                         "IMAGES images: X.ema.png beside every picture, OUT/netG_ema.torch, an \"average\" entry in swd.json; 0: off")
    ap.add_argument("--stats-every", type=int, default=0, metavar="N",
                    help="after every N-th iteration, record per-tensor weight and gradient statistics (OUT/error/EPOCH-stats.npz) "
                         "and stop with an error, before anything is saved, once a weight or gradient is NaN or Inf; 0: off")
    ap.add_argument("--dynamics-every", type=int, default=0, metavar="N",
                    help="around every N-th iteration, record per-tensor update-to-weight ratios and per-layer spectral norms "
                         "(OUT/error/EPOCH-dynamics.npz); 0: off")
    ap.add_argument("--formats-every", type=int, default=0, metavar="N",
                    help="every N-th iteration, audit the operands of every dense contraction against fp8, MX and bf16 formats "
                         "(OUT/error/EPOCH-formats.npz); eager runs only, not with --graph; 0: off")
    ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="X",
                    help="step both networks with GuardedNadam and scale the gradients down to the global L2 norm X where theirs is "
                         "larger (OUT/error/EPOCH-guard.json holds the counters); 0: guard without clipping")
    ap.add_argument("--no-skip-nonfinite", action="store_true",
                    help="step both networks with GuardedNadam but take a step whose gradients hold a NaN or an Inf (it is counted)")
    ap.add_argument("--max-consecutive-skips", type=int, default=16, metavar="N",
                    help="stop with an error, before anything is saved, once a guarded optimizer has skipped N steps in a row")
    ap.add_argument("--rollback-every", type=int, default=0, metavar="N",
                    help="keep a last-good copy of the training state in device memory, renewed once N iterations lie behind the last "
                         "one, and return to it instead of stopping on a NaN or an exhausted guard (OUT/error/rollbacks.json); needs "
                         "--stats-every or a guarded optimizer; 0: off")
    ap.add_argument("--max-rollbacks", type=int, default=3, metavar="N", help="stop as without --rollback-every after N rollbacks")
    ap.add_argument("--spill-every", type=int, default=0, metavar="N",
                    help="write the last-good copy to OUT/spill in the background once N iterations lie behind the last one, and let "
                         "--resume continue from it when it is newer than the last save; needs --rollback-every; 0: off")
    ap.add_argument("--neighbours", type=int, default=0, metavar="IMAGES",
                    help="after every epoch, the nearest training images of the sample picture's images, exact in the 8-bit domain "
                         "(OUT/error/neighbours.json, OUT/error/EPOCH-neighbours.png), against baselines from IMAGES real images; "
                         "one more copy of the training set's canonical views in device memory; 0: off")
    ap.add_argument("--neighbours-k", type=int, default=3, metavar="K", help="nearest training images per sample, 1 .. 8")
    ap.add_argument("--manifold", type=int, default=0, metavar="IMAGES",
                    help="after every epoch, precision, recall, density and coverage of IMAGES generated samples against IMAGES real "
                         "images, exact in the 8-bit domain, with a real-against-real baseline (OUT/error/manifold.json); 0: off")
    ap.add_argument("--manifold-k", type=int, default=3, metavar="K", help="a ball reaches to the K-th nearest other image, 1 .. 8")
    ap.add_argument("--spectrum-images", type=int, default=0, metavar="N",
                    help="after every epoch, the radial power spectrum of N generated samples against N real images, with a "
                         "real-against-real baseline (OUT/error/spectrum.json): the high-frequency excess and the checkerboard of "
                         "up-convolutions; image sizes 32, 64, 128, 256; 0: off")
    ap.add_argument("--spectrum-window", choices=("none", "hann"), default="none",
                    help="window applied to both axes before the transform (none: what the cited papers do)")
    ap.add_argument("--msssim-pairs", type=int, default=0, metavar="N",
                    help="after every epoch, the multi-scale SSIM between N pairs of generated samples beside that of N pairs of real "
                         "images (OUT/error/msssim.json): how alike the samples are, scale by scale; image sizes 32, 64, 128, 256; 0: off")
    ap.add_argument("--modes", type=int, default=0, metavar="SAMPLES",
                    help="after every epoch, the Number of statistically Different Bins of SAMPLES generated samples against the "
                         "k-means cells of real images, exact in the 8-bit domain, with a real-against-real baseline "
                         "(OUT/error/modes.json, OUT/EPOCH-modes.png): which modes are missing; 0: off")
    ap.add_argument("--modes-bins", type=int, default=128, metavar="K", help="k-means cells, 1 .. --modes-images")
    ap.add_argument("--modes-images", type=int, default=16384, metavar="IMAGES", help="real images that are clustered")
    ap.add_argument("--diffaugment", default="", metavar="POLICY",
                    help="differentiable augmentation of every batch the discriminator sees: a comma-separated subset of "
                         "color,translation,cutout (default: off)")
    ap.add_argument("--ada-target", type=float, default=None, metavar="X",
                    help="adaptive augmentation (needs --diffaugment): every op is applied per image with a probability p that rises "
                         "while r_t = E[sign(D(real))] is above X and falls while below (the paper: 0.6); OUT/error/ada.json holds "
                         "the r_t and p curves (default: off, --diffaugment at full strength)")
    ap.add_argument("--ada-kimg", type=float, default=500.0, metavar="K", help="p takes K thousand images from 0 to 1; inf: p stays put")
    ap.add_argument("--ada-interval", type=int, default=4, metavar="N", help="batches per window of r_t")
    ap.add_argument("--ada-initial-p", type=float, default=0.0, metavar="P")
    ap.add_argument("--ada-p-max", type=float, default=1.0, metavar="P")
    ap.add_argument("--lecam", type=float, default=None, metavar="WEIGHT",
                    help="LeCam regularisation of the discriminator: WEIGHT times the mean squared distance of D(real) from the moving "
                         "average of mean D(G(z)) and of D(G(z)) from that of mean D(real) joins the D loss (the paper: 0.3; 0: only "
                         "the two averages are recorded); OUT/error/lecam.json holds their curves (default: off)")
    ap.add_argument("--lecam-decay", type=float, default=0.99, metavar="D", help="decay of the two moving averages")
    ap.add_argument("--lecam-warmup", type=int, default=1000, metavar="N", help="observed iterations before the regulariser switches on")
    ap.add_argument("--lecam-two-sided", action="store_true",
                    help="the paper's equation; default: both distances clamped at 0 before squaring, the released code's form")
    ap.add_argument("--topk-floor", type=float, default=None, metavar="F",
                    help="top-k training of the generator: the G-step's loss runs over the k fakes with the highest D(G(z)), k annealed "
                         "from the batch size down to F times the batch size; OUT/error/topk.json holds the selection's curve "
                         "(default: off)")
    ap.add_argument("--topk-gamma", type=float, default=0.99, metavar="G", help="k's decay per period")
    ap.add_argument("--topk-every", type=int, default=None, metavar="N",
                    help="iterations per period (default: one pass over the image store)")
    return ap


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    if args.neighbours < 0:
        ap.error("--neighbours must be >= 0")
    if not 1 <= args.neighbours_k <= 8:
        ap.error("--neighbours-k must be 1 .. 8")
    if args.manifold < 0:
        ap.error("--manifold must be >= 0")
    if not 1 <= args.manifold_k <= 8:
        ap.error("--manifold-k must be 1 .. 8")
    if args.spectrum_images < 0:
        ap.error("--spectrum-images must be >= 0")
    if args.spectrum_images > 0 and args.image_size not in (32, 64, 128, 256):
        ap.error("--spectrum-images takes --image-size 32, 64, 128 or 256")
    if args.msssim_pairs < 0:
        ap.error("--msssim-pairs must be >= 0")
    if args.msssim_pairs > 0 and args.image_size not in (32, 64, 128, 256):
        ap.error("--msssim-pairs takes --image-size 32, 64, 128 or 256")
    if args.modes < 0 or args.modes_images < 0:
        ap.error("--modes and --modes-images must be >= 0")
    if not 1 <= args.modes_bins <= args.modes_images:
        ap.error("--modes-bins must be 1 .. --modes-images")
    if args.stats_every < 0:
        ap.error("--stats-every must be >= 0")
    if args.dynamics_every < 0:
        ap.error("--dynamics-every must be >= 0")
    if args.formats_every < 0:
        ap.error("--formats-every must be >= 0")
    if args.formats_every > 0 and args.graph:
        ap.error("--formats-every audits eager iterations: a replayed graph runs no Python, so not with --graph")
    if args.clip_grad_norm is not None and not (0.0 <= args.clip_grad_norm < float("inf")):
        ap.error("--clip-grad-norm must be finite and >= 0")
    if args.max_consecutive_skips < 1:
        ap.error("--max-consecutive-skips must be >= 1")
    if args.rollback_every < 0 or args.max_rollbacks < 0:
        ap.error("--rollback-every and --max-rollbacks must be >= 0")
    if args.spill_every < 0:
        ap.error("--spill-every must be >= 0")
    if args.spill_every > 0 and args.rollback_every <= 0:
        ap.error("--spill-every needs --rollback-every: what goes to disk is the last-good copy")
    diffaugment = 0
    if args.diffaugment:
        from .augment import parse_policy
        try:
            diffaugment = parse_policy(args.diffaugment)
        except ValueError as err:
            ap.error("--diffaugment: %s" % err)
        if args.image_size not in (32, 64, 128, 256):
            ap.error("--diffaugment takes --image-size 32, 64, 128 or 256")
    if args.ada_target is not None:
        if not diffaugment:
            ap.error("--ada-target steers --diffaugment's strength: give a --diffaugment policy")
        if not abs(args.ada_target) < float("inf"):
            ap.error("--ada-target must be a finite number")
        if not args.ada_kimg > 0:
            ap.error("--ada-kimg must be > 0 (inf: p stays put)")
        if args.ada_interval < 1:
            ap.error("--ada-interval must be >= 1")
        if not 0.0 < args.ada_p_max <= 1.0:
            ap.error("--ada-p-max must be in (0, 1]")
        if not 0.0 <= args.ada_initial_p <= args.ada_p_max:
            ap.error("--ada-initial-p must be in [0, --ada-p-max]")
    if args.lecam is not None:
        if not abs(args.lecam) < float("inf"):
            ap.error("--lecam must be a finite number")
        if not 0.0 <= args.lecam_decay <= 1.0:
            ap.error("--lecam-decay must be in [0, 1]")
        if not 0 <= args.lecam_warmup < 1 << 31:
            ap.error("--lecam-warmup must be in 0 .. 2^31 - 1")
    if args.topk_floor is not None:
        if not 0.0 <= args.topk_floor <= 1.0:
            ap.error("--topk-floor must be in [0, 1]")
        if not 0.0 < args.topk_gamma <= 1.0:
            ap.error("--topk-gamma must be in (0, 1]")
        if args.topk_every is not None and not 1 <= args.topk_every < 1 << 31:
            ap.error("--topk-every must be in 1 .. 2^31 - 1")
        if not 1 <= args.batch <= 4096:
            ap.error("--topk-floor needs a batch of at most 4096")
    elif args.topk_every is not None or args.topk_gamma != 0.99:
        ap.error("--topk-gamma and --topk-every need --topk-floor")
    guarded_step = args.clip_grad_norm is not None or args.no_skip_nonfinite
    if args.rollback_every > 0 and not (args.stats_every > 0 or guarded_step):
        ap.error("--rollback-every needs --stats-every or a guarded optimizer (--clip-grad-norm / --no-skip-nonfinite): "
                 "nothing else would ever trigger a rollback")

    from . import DeviceImageStore, Discriminator, Generator, InputPipeline, NetConfig, TrainStep, get_model
    from ._lib import require_gpu
    require_gpu()
    dev = torch.device("cuda:0")
    cfg = NetConfig(image_size=args.image_size, seed=args.seed)
    torch.manual_seed(cfg.seed)
    gen, gen_opt = get_model(Generator(cfg), cfg.glr, dev, cfg)
    dis, dis_opt = get_model(Discriminator(cfg), cfg.dlr, dev, cfg)
    if guarded_step:
        from .guard import GuardedNadam
        guarded = dict(max_norm=args.clip_grad_norm or 0.0, skip_nonfinite=not args.no_skip_nonfinite)
        # over get_model's own parameter groups: whatever it sets for Nadam (lr, betas, ...) holds for the guarded step too
        gen_opt = GuardedNadam(gen_opt.param_groups, **guarded)
        dis_opt = GuardedNadam(dis_opt.param_groups, **guarded)
    gen.batched_spectral_norm = dis.batched_spectral_norm = True
    augment = None
    if diffaugment:
        from .augment import AdaptiveDiffAugment, DiffAugment
        if args.ada_target is not None:
            augment = AdaptiveDiffAugment(args.image_size, args.batch, policy=diffaugment, seed=args.seed, device=dev, target=args.ada_target,
                                          interval=args.ada_interval, kimg=args.ada_kimg, initial_p=args.ada_initial_p, p_max=args.ada_p_max)
        else:
            augment = DiffAugment(args.image_size, args.batch, policy=diffaugment, seed=args.seed, device=dev)
    lecam = None
    if args.lecam is not None:
        from .lecam import LeCam
        lecam = LeCam(args.batch, weight=args.lecam, decay=args.lecam_decay, warmup=args.lecam_warmup, one_sided=not args.lecam_two_sided,
                      device=dev)
    pipeline = InputPipeline(DeviceImageStore(args.store, dev), args.image_size, args.batch, seed=args.seed)
    topk = None
    if args.topk_floor is not None:
        from .topk import TopK
        topk = TopK(args.batch, gamma=args.topk_gamma, floor=args.topk_floor, every=args.topk_every or max(1, pipeline.batches_per_epoch),
                    device=dev)
    step = TrainStep(gen, dis, gen_opt, dis_opt, minibatches=args.minibatches, augment=augment, lecam=lecam, topk=topk)
    if not args.resume:
        os.makedirs(args.out, exist_ok=True)

    def log(line):
        sys.stdout.write("\r" + line)
        sys.stdout.flush()

    swd = None
    if args.swd_images > 0:
        from .metric import SlicedWasserstein
        swd = SlicedWasserstein(args.image_size, images=args.swd_images, seed=args.seed, chunk=min(64, args.swd_images), device=dev)
        swd.reference_from_pipeline(pipeline)
    neighbours = None
    if args.neighbours > 0:
        from .neighbours import NearestNeighbours
        neighbours = NearestNeighbours(args.image_size, k=args.neighbours_k, images=args.neighbours, seed=args.seed, device=dev)
        neighbours.reference_from_store(pipeline.store)
    manifold = None
    if args.manifold > 0:
        from .manifold import ManifoldMetrics
        manifold = ManifoldMetrics(args.image_size, k=args.manifold_k, images=args.manifold, seed=args.seed, chunk=min(64, args.manifold),
                                   device=dev)
        manifold.reference_from_store(pipeline.store)
    spectrum = None
    if args.spectrum_images > 0:
        from .spectrum import RadialSpectrum
        spectrum = RadialSpectrum(args.image_size, images=args.spectrum_images, seed=args.seed, chunk=min(64, args.spectrum_images),
                                  window=args.spectrum_window, device=dev)
        spectrum.reference_from_pipeline(pipeline)
    msssim = None
    if args.msssim_pairs > 0:
        from .msssim import MultiScaleSSIM
        msssim = MultiScaleSSIM(args.image_size, pairs=args.msssim_pairs, seed=args.seed, chunk=min(64, 2 * args.msssim_pairs) // 2 * 2, device=dev)
        msssim.reference_from_pipeline(pipeline)
    modes = None
    if args.modes > 0:
        from .modes import BinnedModes
        modes = BinnedModes(args.image_size, bins=args.modes_bins, images=args.modes_images, samples=args.modes, seed=args.seed,
                            chunk=min(64, args.modes), device=dev)
        modes.reference_from_store(pipeline.store)
    average = None
    if args.ema_half_life > 0:
        from .average import AveragedGenerator
        average = AveragedGenerator(gen, half_life_images=args.ema_half_life, batch=args.batch)
    stats = None
    if args.stats_every > 0:
        from .stats import RunStatistics
        stats = RunStatistics(gen, dis)
    dynamics = None
    if args.dynamics_every > 0:
        from .dynamics import RunDynamics
        dynamics = RunDynamics(gen, dis)
    formats = None
    if args.formats_every > 0:
        from .formats import FormatAudit
        formats = FormatAudit(gen, dis)
    snapshot = None
    if args.rollback_every > 0:
        from .snapshot import TrainingSnapshot
        snapshot = TrainingSnapshot(step, average=average)
    trainer = Trainer(step, pipeline, args.out, epochs=args.epochs, max_iterations=args.max_iterations, images=args.images,
                      seed=args.seed, diters=args.diters, graphed=args.graph, log=log, swd=swd, average=average, stats=stats,
                      stats_every=args.stats_every if stats is not None else 16, max_consecutive_skips=args.max_consecutive_skips,
                      snapshot=snapshot, rollback_every=args.rollback_every or 256, max_rollbacks=args.max_rollbacks, spill_every=args.spill_every,
                      dynamics=dynamics, dynamics_every=args.dynamics_every, neighbours=neighbours, manifold=manifold,
                      formats=formats, formats_every=args.formats_every, spectrum=spectrum, msssim=msssim, modes=modes, sampler_options={"advance_spectral_norm": not args.keep_spectral_norm})
    if args.resume:
        trainer.resume()
    else:
        real, aug = InputPipeline(pipeline.store, args.image_size, min(64, len(pipeline.store)), seed=args.seed + 2).next_batch()
        trainer.sampler.preview(real, os.path.join(args.out, "0.png"))          # main.py:45-48
        trainer.sampler.preview(aug, os.path.join(args.out, "1.png"))
    n = trainer.run()
    print("\n%d iterations, state in %s" % (n, args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
