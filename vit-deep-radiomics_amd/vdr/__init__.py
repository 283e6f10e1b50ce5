"""vdr — host side of the MI355X-native ViT dense-descriptor / CLS-feature path.

Importing this package does not touch the GPU; constructing an Engine / model does and raises if
libvdr.so or a HIP device is missing (there is no CPU fallback).
"""
from ._lib import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_TANH, EPI_BIAS_QUICK_GELU, EPI_BIAS_RESID, EPI_SWIGLU, OUT_CLS, OUT_DENSE, OUT_ENCODER,  # noqa: F401
                   OUT_PATCH_EMBED, OUT_POOLED, OUT_TOKENS, VdrError, load, source_id)
from .engine import AttnMap, Engine, FacetOut, LayerOut, VdrConfig  # noqa: F401
from .model import (ARCHS, Correspondences, Cosegmentation, Propagation, TransformerNoduleBimodalClassifier, TransformerNoduleClassifier, VitDescriptorModel, VolumePropagation, extract_dense, get_dense_descriptor,  # noqa: F401
                    load_model)
from . import amg, anomaly, components, kmeans, knn, local, metrics, morphology, pca, pipeline, prep, segment, spectral, upsample  # noqa: F401,E402
from .segment import Segmentation, VolumeSegmentation, segment_slice  # noqa: F401,E402
from .amg import MaskSet  # noqa: F401,E402
from .anomaly import AnomalyMap, Gaussian, GaussianAccumulator, MemoryBank, fit_gaussian  # noqa: F401,E402
from .kmeans import KMeans  # noqa: F401,E402
from .spectral import Lost, TokenCut  # noqa: F401,E402
from .pca import Pca, pca_colorize  # noqa: F401,E402
