"""MI355X-native hot path of GRL image restoration (gfx950 HIP kernels behind the reference's
model boundary).  ``GRL`` takes the reference's constructor arguments and state_dict."""
from .model import GRL  # noqa: F401
from .optim import FusedAdamW  # noqa: F401
from .train_graph import GraphedTrainStep  # noqa: F401
from .presets import baseline_config, make_config  # noqa: F401
from .data import PatchSampler, PatchStore  # noqa: F401
from .train import charbonnier, multistep_warmup_lr  # noqa: F401
from .image8 import ImageWriter, pack8  # noqa: F401
from .restore import restore_folder  # noqa: F401
from .ensemble import SelfEnsemble  # noqa: F401
from .remix import BatchRemix  # noqa: F401
from .discriminator import UNetDiscriminatorSN  # noqa: F401
from .gan import GanStep, gan_loss  # noqa: F401
from .perceptual import PerceptualLoss, VGG19Features, load_vgg19  # noqa: F401

__all__ = ["GRL", "FusedAdamW", "GraphedTrainStep", "make_config", "baseline_config", "PatchStore", "PatchSampler",
           "charbonnier", "multistep_warmup_lr", "pack8", "ImageWriter", "restore_folder", "UNetDiscriminatorSN", "GanStep", "gan_loss",
           "PerceptualLoss", "VGG19Features", "load_vgg19", "SelfEnsemble", "BatchRemix"]
