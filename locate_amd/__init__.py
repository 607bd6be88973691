"""locate_amd: the LocAtE generator/discriminator training step on MI355X (gfx950).

Public names follow the reference's `libs/__init__.py:1-10` for the hot path: NonLinear, BlockBlock,
Generator, Discriminator, SpectralNorm, get_model, hinge-based step (`TrainStep`), parameter_count, Nadam."""
from .config import NetConfig, get_default, set_default  # noqa: F401
from .nn import (ActivatedBaseConv, Block, BlockBlock, CatModule, DeepResidualConv, Expand, FeaturePooling,  # noqa: F401
                 InPlaceNorm, LinearModule, NonLinear, Norm, ResModule, RootTanhModule, Scale, SelfAttention,
                 SpectralNorm, feature_attention)
from .models import Discriminator, Generator, get_model, init, parameter_count  # noqa: F401
from .optim import Nadam  # noqa: F401
from .checkpoint import load_checkpoint, save_checkpoint  # noqa: F401
from .train import TrainLoop, TrainStep  # noqa: F401
from .data import DeviceImageStore, InputPipeline, draw_params, prepare_folder  # noqa: F401
from .monitor import LossHistory, Sampler, image_grid  # noqa: F401
from .metric import (SlicedWasserstein, descriptor_stats, laplacian_pyramid, project_descriptors, pyramid_levels,  # noqa: F401
                     sorted_distance)
from .neighbours import NearestNeighbours, encode_images, nearest  # noqa: F401
from .manifold import ManifoldMetrics, kth_radius, within  # noqa: F401
from .modes import BinnedModes, centroids, group_sums, kmeans_codes, ndb_statistics  # noqa: F401
from .average import AveragedGenerator, average_weight  # noqa: F401
from .augment import AdaptiveDiffAugment, DiffAugment, diff_augment, diff_augment_backward, draw_parameters  # noqa: F401
from .lecam import LeCam  # noqa: F401
from .topk import TopK, topk_k  # noqa: F401
from .stats import NonFiniteError, RunStatistics, tensor_statistics  # noqa: F401
from .dynamics import RunDynamics, tensor_deltas  # noqa: F401
from .formats import FormatAudit, format_errors  # noqa: F401
from .spectrum import RadialSpectrum, dft_tables, radial_bins, radial_spectrum, spectrum_summary  # noqa: F401
from .msssim import MultiScaleSSIM, ms_ssim, ms_ssim_levels, ms_ssim_value, window_taps  # noqa: F401
from .guard import GuardedNadam, GuardExhausted  # noqa: F401
from .snapshot import NoSnapshot, StateSnapshot, TrainingSnapshot, arena_layout  # noqa: F401
from .spill import (SnapshotSpill, SpillCorrupt, SpillMismatch, digest_model, read_spill, restore_training_state,  # noqa: F401
                    tensor_digests, write_spill)


def __getattr__(name):
    # `Trainer` is resolved on first use, so that `python -m locate_amd.run` does not find its module imported already
    if name == "Trainer":
        from .run import Trainer
        return Trainer
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
