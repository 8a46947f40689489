"""polyblur_amd -- MI355X-native Polyblur blind deblurring (drop-in for teboli/polyblur's
``polyblur_deblurring`` / ``PolyblurDeblurring``; reference polyblur/__init__.py:1).

The compute path is hand-written HIP for gfx950 behind the C ABI in
``include/polyblur_hip.h`` (``libpolyblur_hip.so``), loaded lazily with ctypes on the
first call.  There is no CPU fallback: without the library or a GPU the calls raise.
"""
from .deblurring import polyblur_deblurring, polyblur_deblurring_uint8, PolyblurDeblurring  # noqa: F401
# the non-blind step with a kernel of the caller's (reference deblurring.py:211-239, filters.py:14-37, edgetaper.py:26-33);
# all three differentiable with respect to the image and the kernel, the edgetaper through its weights too
from .nonblind import inverse_filtering_rank3, convolve2d, edgetaper  # noqa: F401
# ... and for kernels that are not point-symmetric: the pure-phase filter (reference deblurring.py:113-169, not_symmetric=True),
# differentiable with respect to the image and the kernel like the three above
from .nonblind import compute_polynomial, inverse_filtering_nonsymmetric  # noqa: F401
# the blind estimation itself, differentiable (reference blur_estimation.py:18-79)
from .estimation import gaussian_blur_estimation  # noqa: F401
# halo masking and the spectral derivative, differentiable (reference deblurring.py:193-208, filters.py:159-186)
from .halo import fourier_gradients, halo_masking  # noqa: F401
# the edge-aware filters behind prefiltering=True; the bilateral filter and the recursive filter (image and guide) are
# differentiable, the normalized convolution is forward only
# (reference filters.py:107-148, domain_transform.py:6-85, deblurring.py:99-110)
from .edge_aware import bilateral_filter, recursive_filter, normalized_convolution, edge_aware_filtering  # noqa: F401
# the two ends of the patch decomposition, differentiable (reference deblurring.py:269-340, fix-forward)
from .patches import image_to_patches, patches_to_image  # noqa: F401

__all__ = ["polyblur_deblurring", "polyblur_deblurring_uint8", "PolyblurDeblurring",
           "inverse_filtering_rank3", "convolve2d", "edgetaper", "compute_polynomial", "inverse_filtering_nonsymmetric",
           "gaussian_blur_estimation", "fourier_gradients", "halo_masking",
           "bilateral_filter", "recursive_filter", "normalized_convolution", "edge_aware_filtering",
           "image_to_patches", "patches_to_image"]
__version__ = "0.1.0"
