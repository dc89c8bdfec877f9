"""MI355X-native UNet segmentation train-step path (hand-written HIP kernels behind the reference's
nn.Module / loss-function surface).  See DESIGN.md and include/unet_hip.h."""
from .unet import UNet, UNet_S, UNet_SA, UNet_T, UNetDepth, DoubleConv, Down, Up, OutConv  # noqa: F401
from .unet import AttentionUp, SpatialAttention  # noqa: F401
from .utils.dice_score import dice_coeff, multiclass_dice_coeff, dice_loss  # noqa: F401
from .utils.boundary_loss import boundary_loss  # noqa: F401
from .utils.connected_component_loss import connected_component_loss  # noqa: F401
from .utils.surface_loss import surface_loss, surface_distance_map  # noqa: F401
from .utils.focal_loss import LossConfig, focal_tversky_loss  # noqa: F401
from .utils.distill import DistillConfig, Distiller, distill_loss  # noqa: F401
from .train import FusedRMSprop, seg_loss, train_step, TrainStepper, GraphedTrainStepper, EmaConfig  # noqa: F401
from .train import OptimConfig, FusedOptimizer, FusedAdamW, FusedSGD  # noqa: F401
from .evaluate import evaluate  # noqa: F401
from .utils.contour_metrics import contour_metrics, ContourMetrics  # noqa: F401
from .predict import predict_img, mask_to_image, preprocess_image, BatchPredictor, plan_batches  # noqa: F401
from .checkpoint import save_checkpoint, load_checkpoint  # noqa: F401
from .synthetic import ellipse_batch  # noqa: F401
from .utils.data_loading import BasicDataset, CarvanaDataset, load_image  # noqa: F401
from .utils.augment import AugmentConfig, BatchAugment, ElasticConfig  # noqa: F401
from .utils.post_process import postprocess_mask, remove_internal_regions  # noqa: F401
from .utils.tta import tta_mask, tta_view_shape, tta_source_position  # noqa: F401
from .utils.tiling import TileConfig, parse_tile_spec, tile_grid  # noqa: F401
from .utils.crop import CropConfig, BatchCrop  # noqa: F401
from .utils.dataset_cache import DatasetCache, DatasetCacheTooLarge, plan_entries  # noqa: F401
from .utils.ensemble import Ensemble, MemberSpec, parse_member_spec  # noqa: F401
from .inference import GraphedForward  # noqa: F401
from .utils.raw2png import read_raw, window_level  # noqa: F401
from .utils.png_normalize import letterbox, letterbox_geometry, lanczos_coeffs  # noqa: F401
from .utils.png_denormalize import unletterbox  # noqa: F401
from .utils.mask2polygon import external_contours, contour_json  # noqa: F401
from .seg_main import ContourPipeline  # noqa: F401
