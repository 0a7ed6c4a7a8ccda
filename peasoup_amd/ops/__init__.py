"""PyTorch-ROCm facing wrappers of the hand-written HIP kernels.

Every op takes/returns ``torch`` tensors on the current HIP device and runs on
``torch.cuda.current_stream()``, so it composes with torch code and graph
capture.  The native extension must be loaded: there is no silent CPU
fallback (a missing/unbuilt extension raises at import).
"""
from .core import (  # noqa: F401
    FFTPlanCache,
    coincidence_counts,
    coincidence_mask,
    conjugate,
    cmul_,
    convert_pad,
    dedisperse,
    deredden,
    fft4_resample_interbin,
    fft4_spectrum_pass,
    spec_unblock,
    spec_pblk_index,
    fft4_resample_spectrum,
    burst_cube,
    fold_cube,
    fold_optimise,
    fold_raw,
    fold_series,
    form_amplitude,
    form_interbin,
    harmonic_peaks,
    harmonic_sums,
    interbin_normalise,
    interbin_stats,
    irfft,
    median_scrunch5,
    normalise,
    pack_transpose,
    quantize_q8,
    r2c_interbin_normalise,
    resample,
    rfi_apply,
    rfi_block_sums,
    rfi_clean,
    rfi_tile,
    resample_v1,
    rfft,
    running_median,
    single_pulse_search,
    unpack_transpose,
)
