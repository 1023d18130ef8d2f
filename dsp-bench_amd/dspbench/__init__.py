"""dspbench -- MI355X-native offline render + spectrum path for DSP-Bench plugins.

All compute runs in libdspbench.so (HIP kernels for gfx950).  See DESIGN.md.
"""
from ._lib import (DSP_WIN_HAMMING, DSP_WIN_HANN, DSP_WIN_RECT, DspError, LIB_PATH,  # noqa: F401
                   lib)
from .api import (IR_BUFFER_LENGTH, Plugin, conv_plan, deconv_plan, deconvolve, fft_forward, fft_reverse, ir_analysis,  # noqa: F401
                  k_weighting, limiter, limiter_plan, loudness, loudness_gate, loudness_plan, minmax_decimate, num_blocks,
                  render_loop, render_offline, render_stft, render_stft_host,
                  resample, resample_plan, resample_taps, irfft, rfft, rfft_plan, spectrogram_decimate,
                  stft_frames, stft_magnitude, sweep, sweep_harmonic_offset, sweep_plan,
                  csd, transfer, welch, welch_derive, welch_plan, welch_sums,
                  istft, istft_plan, stft, stft_plan,
                  phase_vocoder, pitch_ratio, pitch_shift, pitch_shift_plan, pvoc_plan, time_stretch, time_stretch_plan,
                  decay, decay_derive, decay_energies, decay_plan)
from . import module, shard, wav  # noqa: F401

__all__ = ["Plugin", "render_offline", "render_loop", "render_stft_host", "minmax_decimate", "spectrogram_decimate", "stft_magnitude", "render_stft", "ir_analysis",
           "fft_forward", "fft_reverse", "conv_plan", "resample", "resample_plan", "resample_taps", "stft_frames", "num_blocks", "lib", "DspError",
           "loudness", "loudness_plan", "loudness_gate", "k_weighting", "limiter", "limiter_plan",
           "rfft", "irfft", "rfft_plan", "deconvolve", "deconv_plan", "sweep", "sweep_plan", "sweep_harmonic_offset",
           "welch", "csd", "transfer", "welch_plan", "welch_sums", "welch_derive",
           "stft", "istft", "stft_plan", "istft_plan",
           "phase_vocoder", "pvoc_plan", "time_stretch", "time_stretch_plan", "pitch_ratio", "pitch_shift", "pitch_shift_plan",
           "decay", "decay_plan", "decay_energies", "decay_derive",
           "DSP_WIN_HAMMING", "DSP_WIN_HANN", "DSP_WIN_RECT", "IR_BUFFER_LENGTH", "shard", "wav", "module"]
