"""Host-side helpers that sit on the hot path's boundary (enums, transforms, pair selection)."""
from .enums import (InterpMode, MissingStdMode, VarianceMode, ChannelOrder, DimensionOrder, DTYPE_MAP,
                    REVERSE_DTYPE_MAP)
from .typecheck import TypeCheckError
from .statistics import WBOMean, WBOMeanVar
from .data_io import load_icrf_txt, save_icrf_txt, image_to_cv_array, save_image
from .general_functions import (get_valid_exposure_pairs, get_pairwise_valid_pixel_mask, weighted_mean_and_std,
                                flat_field_mean, flatfield_correction, cv_to_torch, torch_to_cv, normalize_tensor,
                                clamp_along_dims)
from .transforms import (BaseTransform, CvToTorch, TorchToCv, CastTo, Normalize, ClampAlongDims, StridedDownscale,
                         fusable_layout, fusable_code_normalisation, fusable_downscale)
