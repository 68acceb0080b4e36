"""vq_amd -- MI355X (gfx950) back end for the k-means codebook-training and nearest-centroid
encode path of CogitatorTech/vq, and of its elementwise scalar / binary quantizers, behind the
reference's own Quantizer interface, exact k-NN search over resident rows (FlatIndex), an inverted-file
index over PQ codes (IVFPQIndex) one over the rows themselves (IVFFlatIndex) and one over SQ codes
(IVFScalarIndex), one over the same codes at four bits a dimension (IVFScalar4Index) and one over packed BQ bits (IVFBinaryIndex), a Hamming index over packed BQ codes (BinaryIndex), an exact index over
resident SQ codes (ScalarIndex), one over the same codes at four bits a dimension (Scalar4Index) and an exact index of f32 queries over packed BQ bits (AsymmetricBinaryIndex).

The compute path is libvqhip.so (hand-written HIP for CDNA4, C ABI in include/vqhip.h).
Importing the package does not need a GPU; using any quantizer does, and fails loudly
(``FfiError``) otherwise -- there is no CPU fallback.
"""
from .distance import Distance
from .errors import (DimensionMismatch, EmptyInput, FfiError, InvalidData, InvalidParameter,
                     VqError)
from .asymmetric_binary import AsymmetricBinaryIndex
from .binary import BinaryIndex
from .bq import BinaryQuantizer
from ._lib import RangeResult
from ._resident_common import pack_row_mask
from .flat import FlatIndex
from .ivf import IVFPQIndex
from .ivf_flat import IVFFlatIndex
from .ivf_binary import IVFBinaryIndex
from .ivf_scalar import IVFScalarIndex
from .ivf_scalar4 import IVFScalar4Index
from .pq import ProductQuantizer, fit_codebooks
from .scalar4_index import Scalar4Index
from .scalar_index import ScalarIndex
from .sq import ScalarQuantizer
from .tsvq import TSVQ

__all__ = [
    "Distance", "AsymmetricBinaryIndex", "BinaryIndex", "BinaryQuantizer", "FlatIndex", "IVFBinaryIndex", "IVFFlatIndex", "IVFPQIndex", "IVFScalar4Index", "IVFScalarIndex", "RangeResult", "Scalar4Index", "ScalarIndex", "ScalarQuantizer", "ProductQuantizer", "TSVQ", "fit_codebooks", "VqError", "DimensionMismatch", "EmptyInput",
    "InvalidParameter", "InvalidData", "FfiError", "get_simd_backend", "pack_row_mask",
]


def get_simd_backend() -> str:
    """pyvq.get_simd_backend analogue (pyvq/src/lib.rs:19-21): names the active back end."""
    from . import _lib

    return _lib.backend()
