"""ctypes binding of libdspbench.so (include/dspbench/dspbench.h, host.h, wav.h, module.h).

The library is the product: there is no Python or CPU fallback behind these
functions.  If the shared object is missing the import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # dsp-bench_amd/
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.environ.get("DSPBENCH_LIB", os.path.join(PKG_ROOT, "libdspbench.so"))

DSP_OK = 0
DSP_ERR_INVALID = -1
DSP_ERR_HIP = -2
DSP_ERR_UNSUPPORTED = -3
DSP_ERR_NOMEM = -4
DSP_ERR_NO_DEVICE = -5

DSP_WIN_HAMMING, DSP_WIN_HANN, DSP_WIN_RECT = 0, 1, 2

DSP_PLUGIN_NOOP = 0
DSP_PLUGIN_GAIN = 1
DSP_PLUGIN_STATIC_GAIN = 2
DSP_PLUGIN_IR_RAMP = 3
DSP_PLUGIN_FIR = 4
DSP_PLUGIN_BIQUAD = 5
DSP_PLUGIN_CONV = 6
DSP_PLUGIN_GENERIC = 16

DSP_EXEC_HOST_BUFFERS = 0x1
DSP_EXEC_SYNC = 0x2
DSP_EXEC_FIR_DIRECT = 0x4
DSP_EXEC_NO_SPECIALIZE = 0x8
DSP_EXEC_VERIFY_CLASS = 0x10
DSP_EXEC_SERIAL_STATE = 0x20
DSP_EXEC_EVERY_FRAME = 0x40
DSP_EXEC_METHOD_FLAGS = (DSP_EXEC_FIR_DIRECT | DSP_EXEC_NO_SPECIALIZE | DSP_EXEC_VERIFY_CLASS |
                         DSP_EXEC_SERIAL_STATE | DSP_EXEC_EVERY_FRAME)
DSP_RESULT_CLASS = 0x1
DSP_RESULT_VERIFIED = 0x2
DSP_RESULT_RERENDERED = 0x4
DSP_RESULT_FRAME_REUSE = 0x8
DSP_DEBUG_FRAME_RUN = 3  # dsp_debug_set / _get: frames per wave of the frame reuse (test hook)
DSP_BLOCK_CALLBACK, DSP_BLOCK_TABLE, DSP_BLOCK_GAIN, DSP_BLOCK_GAIN_TABLE = 0, 1, 2, 3


class DspError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str):
        super().__init__(f"{what}: status {status} ({detail})")
        self.status = status


class dsp_plugin(C.Structure):
    _fields_ = [("kind", C.c_int32), ("params_size", C.c_uint32), ("params", C.c_void_p),
                ("state_size", C.c_uint32), ("state", C.c_void_p), ("module", C.c_void_p)]


class dsp_exec(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32), ("stream", C.c_void_p),
                ("sample_offset", C.c_uint64), ("result", C.POINTER(C.c_uint32))]


class dsp_resample_spec(C.Structure):
    _fields_ = [("zeros", C.c_uint32), ("beta", C.c_double), ("rolloff", C.c_double)]


class dsp_loudness_result(C.Structure):
    _fields_ = [("integrated", C.c_double), ("range", C.c_double), ("momentary_max", C.c_double),
                ("short_term_max", C.c_double), ("sample_peak", C.c_double), ("true_peak", C.c_double),
                ("blocks", C.c_uint64), ("gated_blocks", C.c_uint64)]


DSP_LOUDNESS_TRUE_PEAK = 0x1


class dsp_limiter_spec(C.Structure):
    _fields_ = [("ceiling", C.c_float), ("lookahead", C.c_uint32), ("release", C.c_double), ("flags", C.c_uint32)]


class dsp_limiter_result(C.Structure):
    _fields_ = [("min_gain", C.c_double), ("limited", C.c_uint64)]


DSP_LIMITER_UNLINKED = 0x1
DSP_LIMITER_TRUE_PEAK = 0x2


class dsp_deconv_spec(C.Structure):
    _fields_ = [("eps", C.c_double), ("pre", C.c_uint32)]


class dsp_sweep_spec(C.Structure):
    _fields_ = [("f1", C.c_double), ("f2", C.c_double), ("seconds", C.c_double), ("amplitude", C.c_double),
                ("fade", C.c_uint32)]


class dsp_welch_spec(C.Structure):
    _fields_ = [("N", C.c_uint32), ("H", C.c_uint32), ("window", C.c_int32)]


DSP_WELCH_SPECTRUM = 0x1


class dsp_stft_spec(C.Structure):
    _fields_ = [("N", C.c_uint32), ("H", C.c_uint32), ("window", C.c_int32)]


class dsp_istft_spec(C.Structure):
    _fields_ = [("N", C.c_uint32), ("H", C.c_uint32), ("window", C.c_int32), ("floor", C.c_double)]


class dsp_pvoc_spec(C.Structure):
    _fields_ = [("rate", C.c_double)]


class dsp_stretch_spec(C.Structure):
    _fields_ = [("rate", C.c_double), ("N", C.c_uint32), ("H", C.c_uint32), ("window", C.c_int32),
                ("floor", C.c_double)]


class dsp_decay_spec(C.Structure):
    _fields_ = [("fraction", C.c_uint32), ("k_lo", C.c_int32), ("k_hi", C.c_int32)]


class dsp_decay_result(C.Structure):
    _fields_ = [("edt", C.c_double), ("t20", C.c_double), ("t30", C.c_double), ("c50", C.c_double),
                ("c80", C.c_double), ("d50", C.c_double), ("ts", C.c_double), ("inr", C.c_double),
                ("flags", C.c_uint32), ("truncation", C.c_uint32), ("reserved", C.c_uint32 * 2)]


DSP_DECAY_SILENT = 0x1
DSP_DECAY_EDT_INVALID = 0x2
DSP_DECAY_T20_INVALID = 0x4
DSP_DECAY_T30_INVALID = 0x8
DSP_DECAY_SHORT = 0x10

DPP = C.POINTER(C.POINTER(C.c_double))
DP = C.POINTER(C.c_double)

DSP_WAV_FORMAT_PCM = 1
DSP_WAV_FORMAT_FLOAT = 3
DSP_WAV_MAX_DATA_CHUNKS = 8


class dsp_wav_info(C.Structure):
    _fields_ = [("format", C.c_uint16), ("channels", C.c_uint16), ("sample_rate", C.c_uint32),
                ("bits_per_sample", C.c_uint16), ("block_align", C.c_uint16), ("frames", C.c_uint64),
                ("data_bytes", C.c_uint64), ("n_data_chunks", C.c_uint32),
                ("data_offset", C.c_uint64 * DSP_WAV_MAX_DATA_CHUNKS),
                ("data_size", C.c_uint64 * DSP_WAV_MAX_DATA_CHUNKS)]


FPP = C.POINTER(C.POINTER(C.c_float))
FP = C.POINTER(C.c_float)

DSP_PARAM_INT, DSP_PARAM_FLOAT, DSP_PARAM_ENUM = 0, 1, 2
DSP_PARAM_NAME_MAX = 64


class dsp_param_desc(C.Structure):
    _fields_ = [("name", C.c_char * DSP_PARAM_NAME_MAX), ("offset", C.c_uint32), ("type", C.c_int32),
                ("error", C.c_int32), ("int_min", C.c_int32), ("int_max", C.c_int32),
                ("float_min", C.c_float), ("float_max", C.c_float), ("float_log", C.c_int32),
                ("num_entries", C.c_uint32)]


class dsp_plugin_descriptor(C.Structure):
    _fields_ = [("params_size", C.c_uint64), ("params_align", C.c_uint64), ("state_size", C.c_uint64),
                ("state_align", C.c_uint64), ("num_parameters", C.c_uint32), ("error", C.c_int32)]


class dsp_param_value(C.Union):
    _fields_ = [("int_value", C.c_int32), ("float_value", C.c_float), ("enum_value", C.c_int32)]


class dsp_callback_facts(C.Structure):  # module.h
    _fields_ = [("present", C.c_int32), ("analyzed", C.c_int32), ("reads_block", C.c_int32),
                ("writes_state", C.c_int32), ("input_control", C.c_int32), ("gain_form", C.c_int32),
                ("gain_source", C.c_int32), ("gain_offset", C.c_uint32), ("gain_constant", C.c_float),
                ("gain", C.c_char * 128), ("why", C.c_char * 256), ("gain_table_form", C.c_int32),
                ("table_why", C.c_char * 128), ("state_reads_block", C.c_int32), ("state_split", C.c_int32),
                ("state_dep_words", C.c_char * 64)]

    def as_dict(self) -> dict:
        return {"present": bool(self.present), "analyzed": bool(self.analyzed),
                "reads_block": bool(self.reads_block), "writes_state": bool(self.writes_state),
                "input_control": bool(self.input_control), "gain_form": bool(self.gain_form),
                "gain_source": chr(self.gain_source) if self.gain_source else "",
                "gain_offset": int(self.gain_offset), "gain_constant": float(self.gain_constant),
                "gain": self.gain.decode(errors="replace"), "why": self.why.decode(errors="replace"),
                "gain_table_form": bool(self.gain_table_form),
                "table_why": self.table_why.decode(errors="replace"),
                "state_reads_block": bool(self.state_reads_block), "state_split": bool(self.state_split),
                "state_dep_words": self.state_dep_words.decode(errors="replace")}


class dsp_state_spec_info(C.Structure):  # module.h
    _fields_ = [("used", C.c_int32), ("disabled", C.c_int32), ("segments", C.c_uint32),
                ("blocks_per_segment", C.c_uint32), ("warmup_blocks", C.c_uint32), ("differed", C.c_uint32 * 3),
                ("serial_reruns", C.c_uint32), ("levels", C.c_uint32), ("chain", C.c_int32),
                ("chain_mismatch", C.c_uint32), ("chain_records_differed", C.c_uint32), ("split", C.c_int32)]

    def as_dict(self) -> dict:
        return {"used": bool(self.used), "disabled": bool(self.disabled), "segments": int(self.segments),
                "blocks_per_segment": int(self.blocks_per_segment), "warmup_blocks": int(self.warmup_blocks),
                "differed": [int(v) for v in self.differed], "serial_reruns": int(self.serial_reruns),
                "levels": int(self.levels), "chain": bool(self.chain),
                "chain_mismatch": int(self.chain_mismatch),
                "chain_records_differed": int(self.chain_records_differed), "split": bool(self.split)}


# name -> (restype, argtypes)
_SIGS = {
    "dsp_abi_version": (C.c_int, []),
    "dsp_status_string": (C.c_char_p, [C.c_int]),
    "dsp_last_error": (C.c_char_p, []),
    "dsp_device_count": (C.c_int, []),
    "dsp_stft_frame_count": (C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint32]),
    "dsp_conv_plan": (C.c_int, [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "dsp_resample_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(dsp_resample_spec),
                                    C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "dsp_resample_taps": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(dsp_resample_spec), FP, C.c_uint64]),
    "dsp_resample": (C.c_int, [FPP, C.c_uint32, C.c_uint64, FPP, C.c_uint64, C.c_uint32, C.c_uint32,
                               C.POINTER(dsp_resample_spec), C.POINTER(dsp_exec)]),
    "dsp_loudness_plan": (C.c_int, [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint32), FP, C.POINTER(C.c_uint64)]),
    "dsp_loudness_gate": (C.c_int, [DPP, C.c_uint32, C.c_uint64, C.c_uint32, FP, C.POINTER(dsp_loudness_result)]),
    "dsp_loudness": (C.c_int, [FPP, C.c_uint32, C.c_uint64, C.c_uint32, FP, C.c_uint32,
                               C.POINTER(dsp_resample_spec), DPP, C.POINTER(C.c_double),
                               C.POINTER(dsp_loudness_result), C.POINTER(dsp_exec)]),
    "dsp_limiter_plan": (C.c_int, [C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(dsp_limiter_spec),
                                   C.POINTER(dsp_resample_spec), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), FP, FP,
                                   C.POINTER(C.c_uint64)]),
    "dsp_limiter": (C.c_int, [FPP, C.c_uint32, C.c_uint64, FPP, C.c_uint32, C.POINTER(dsp_limiter_spec),
                              C.POINTER(dsp_resample_spec), FPP, FPP, C.POINTER(dsp_limiter_result),
                              C.POINTER(dsp_exec)]),
    "dsp_rfft_plan": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "dsp_rfft": (C.c_int, [FPP, C.c_uint32, C.c_uint64, C.c_uint32, FPP, C.POINTER(dsp_exec)]),
    "dsp_irfft": (C.c_int, [FPP, C.c_uint32, C.c_uint32, FPP, C.c_uint64, C.POINTER(dsp_exec)]),
    "dsp_deconv_plan": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "dsp_deconvolve": (C.c_int, [FPP, C.c_uint32, C.c_uint64, FP, C.c_uint64, FPP, C.c_uint64,
                                 C.POINTER(dsp_deconv_spec), C.POINTER(dsp_exec)]),
    "dsp_sweep_plan": (C.c_int, [C.c_uint32, C.POINTER(dsp_sweep_spec), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "dsp_sweep": (C.c_int, [C.c_uint32, C.POINTER(dsp_sweep_spec), FP, C.c_uint64]),
    "dsp_sweep_harmonic_offset": (C.c_int, [C.c_uint32, C.POINTER(dsp_sweep_spec), C.c_uint32, C.POINTER(C.c_double)]),
    "dsp_welch_plan": (C.c_int, [C.c_uint64, C.c_uint32, C.c_int, C.POINTER(dsp_welch_spec), C.POINTER(C.c_uint64),
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), DP, DP]),
    "dsp_welch": (C.c_int, [FPP, C.c_uint32, C.c_uint64, FP, DPP, DP, DPP, C.POINTER(dsp_welch_spec),
                            C.POINTER(dsp_exec)]),
    "dsp_welch_derive": (C.c_int, [DPP, DP, DPP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_double, C.c_double,
                                   C.c_double, C.c_uint32, DPP, DPP, DPP]),
    "dsp_stft_plan": (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(dsp_stft_spec), C.POINTER(C.c_uint64),
                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "dsp_stft": (C.c_int, [FPP, C.c_uint32, C.c_uint64, FPP, C.c_uint64, C.POINTER(dsp_stft_spec), C.POINTER(dsp_exec)]),
    "dsp_istft_plan": (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(dsp_istft_spec), C.POINTER(C.c_uint64),
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "dsp_istft": (C.c_int, [FPP, C.c_uint32, C.c_uint64, C.c_uint64, FPP, C.c_uint64, C.POINTER(dsp_istft_spec),
                            C.POINTER(dsp_exec)]),
    "dsp_pvoc_plan": (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(dsp_pvoc_spec), C.POINTER(C.c_uint64),
                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "dsp_pvoc": (C.c_int, [FPP, C.c_uint32, C.c_uint64, C.c_uint64, FPP, C.c_uint64, C.POINTER(dsp_pvoc_spec),
                           C.POINTER(dsp_exec)]),
    "dsp_time_stretch_plan": (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(dsp_stretch_spec), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64)]),
    "dsp_time_stretch": (C.c_int, [FPP, C.c_uint32, C.c_uint64, FPP, C.c_uint64, C.POINTER(dsp_stretch_spec),
                                   C.POINTER(dsp_exec)]),
    "dsp_pitch_ratio": (C.c_int, [C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "dsp_pitch_shift_plan": (C.c_int, [C.c_uint64, C.c_uint32, C.c_double, C.c_uint32, C.c_int32, C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32), C.POINTER(dsp_stretch_spec), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "dsp_decay_plan": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(dsp_decay_spec), C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), DP]),
    "dsp_decay": (C.c_int, [FPP, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(dsp_decay_spec), FP,
                            C.POINTER(C.c_uint64), DPP, DPP, C.POINTER(dsp_exec)]),
    "dsp_decay_derive": (C.c_int, [DP, DP, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                   C.POINTER(dsp_decay_result)]),
    "dsp_render_offline": (C.c_int, [FPP, C.c_uint32, C.c_uint64, FPP, C.c_uint32, C.c_uint32,
                                     C.c_float, C.POINTER(dsp_plugin), C.POINTER(dsp_exec)]),
    "dsp_render_loop": (C.c_int, [FPP, C.c_uint32, C.c_uint64, C.c_uint64, FPP, C.c_uint32, C.c_uint32,
                                  C.c_uint64, C.c_float, C.POINTER(dsp_plugin), C.POINTER(C.c_uint64),
                                  C.POINTER(dsp_exec)]),
    "dsp_stft_magnitude": (C.c_int, [FPP, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                     C.c_int32, C.c_uint32, FPP, C.c_uint64, C.POINTER(dsp_exec)]),
    "dsp_render_stft": (C.c_int, [FPP, C.c_uint32, C.c_uint64, FPP, C.c_uint32, C.c_uint32,
                                  C.c_float, C.POINTER(dsp_plugin), C.c_uint32, C.c_uint32,
                                  C.c_int32, C.c_uint32, FPP, C.c_uint64, C.POINTER(dsp_exec)]),
    "dsp_render_stft_host": (C.c_int, [FPP, C.c_uint32, C.c_uint64, FPP, C.c_uint32, C.c_uint32, C.c_float,
                                       C.POINTER(dsp_plugin), C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, FPP,
                                       C.c_uint64, C.c_uint64, C.POINTER(dsp_exec)]),
    "dsp_ir_analysis": (C.c_int, [C.POINTER(dsp_plugin), C.c_uint32, C.c_float, C.c_uint32,
                                  FPP, FP, C.POINTER(dsp_exec)]),
    "dsp_fft_forward": (C.c_int, [FP, FP, FP, C.c_uint32, C.POINTER(dsp_exec)]),
    "dsp_fft_reverse": (C.c_int, [FP, FP, FP, C.c_uint32, C.POINTER(dsp_exec)]),
    "dsp_gain": (C.c_int, [FP, FP, C.c_float, C.c_uint64, C.POINTER(dsp_exec)]),
    "dsp_copy": (C.c_int, [FP, FP, C.c_uint64, C.POINTER(dsp_exec)]),
    "dsp_set": (C.c_int, [C.c_float, FP, C.c_uint64, C.POINTER(dsp_exec)]),
    "dsp_magnitude": (C.c_int, [FP, FP, FP, C.c_uint64, C.POINTER(dsp_exec)]),
    "dsp_kernel_timing_enable": (None, [C.c_int]),
    "dsp_kernel_timing": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "dsp_initializer_create": (C.c_void_p, [C.c_size_t, C.c_int]),
    "dsp_initializer_reset": (None, [C.c_void_p]),
    "dsp_initializer_used": (C.c_size_t, [C.c_void_p]),
    "dsp_initializer_destroy": (None, [C.c_void_p]),
    "dsp_host_report": (None, [C.c_char_p, C.c_int]),
    "dsp_minmax_decimate": (C.c_int, [FP, C.c_uint64, C.c_uint32, FP, FP, C.POINTER(dsp_exec)]),
    "dsp_spectrogram_decimate": (C.c_int, [FP, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, FP,
                                           C.POINTER(dsp_exec)]),
    "dsp_module_compile": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                     C.c_char_p, C.c_uint64]),
    "dsp_module_free_code": (None, [C.c_void_p]),
    "dsp_module_load": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]),
    "dsp_module_destroy": (None, [C.c_void_p]),
    "dsp_module_sizes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_int)]),
    "dsp_module_default_parameters": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dsp_module_initialize_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint64]),
    "dsp_module_read_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dsp_module_block_class": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(dsp_exec)]),
    "dsp_module_facts": (C.c_int, [C.c_void_p, C.POINTER(dsp_callback_facts)]),
    "dsp_module_state_spec": (C.c_int, [C.c_void_p, C.POINTER(dsp_state_spec_info)]),
    "dsp_plugin_analyze": (C.c_int, [C.c_char_p, C.POINTER(dsp_callback_facts)]),
    "dsp_code_facts": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(dsp_callback_facts)]),
    "dsp_descriptor_from_code": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "dsp_descriptor_destroy": (None, [C.c_void_p]),
    "dsp_module_descriptor": (C.c_void_p, [C.c_void_p]),
    "dsp_descriptor_info": (C.c_int, [C.c_void_p, C.POINTER(dsp_plugin_descriptor)]),
    "dsp_descriptor_param": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(dsp_param_desc)]),
    "dsp_descriptor_enum_entry": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64),
                                            C.c_char_p, C.c_uint32]),
    "dsp_params_from_values": (C.c_int, [C.c_void_p, C.POINTER(dsp_param_value), C.c_void_p]),
    "dsp_params_to_values": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(dsp_param_value)]),
    "dsp_descriptor_equal": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dsp_param_normalize": (C.c_int, [C.POINTER(dsp_param_desc), C.POINTER(C.c_int64), dsp_param_value,
                                      C.POINTER(C.c_float)]),
    "dsp_param_denormalize": (C.c_int, [C.POINTER(dsp_param_desc), C.POINTER(C.c_int64), C.c_float,
                                        C.POINTER(dsp_param_value)]),
    "dsp_wav_parse": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(dsp_wav_info)]),
    "dsp_wav_decode": (C.c_int, [C.c_void_p, C.POINTER(dsp_wav_info), C.c_uint64, C.c_uint64, FPP,
                                 C.POINTER(dsp_exec)]),
    "dsp_wav_encode": (C.c_int, [FPP, C.c_uint32, C.c_uint64, C.c_uint16, C.c_uint16, C.c_void_p,
                                 C.POINTER(dsp_exec)]),
    "dsp_render_stft_wav": (C.c_int, [C.c_void_p, C.POINTER(dsp_wav_info), C.c_uint32, C.c_uint32, C.c_float,
                                      C.POINTER(dsp_plugin), C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, FPP, FPP,
                                      C.c_uint64, C.c_uint64, C.POINTER(dsp_exec)]),
    "dsp_wav_write_header": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint16, C.c_uint16, C.c_uint32,
                                       C.c_uint16, C.c_uint64]),
}

# exported only by the A/B tools build (build/ab/libdspbench_ab.so)
_OPTIONAL_SIGS = {
    # test hooks and diagnostics (an A/B library built from an older tree may lack them)
    "dsp_debug_set": (C.c_int, [C.c_int, C.c_uint64]),
    "dsp_debug_get": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "dsp_module_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64]),
    "dsp_ir_strip_chain_stores": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_int32)]),
    "dsp_plugin_analyze_shipped": (C.c_int, [C.c_char_p, C.POINTER(dsp_callback_facts)]),
    "dsp_module_seg_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "dsp_stft_pk_ab_options": (C.c_int, [C.c_int]),
}

_lib: C.CDLL | None = None


ABI_VERSION = 3  # include/dspbench/dspbench.h DSPBENCH_ABI_VERSION this binding is written against


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libdspbench.so not built at {LIB_PATH} "
                              "(run `make -C dsp-bench_amd` or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in _OPTIONAL_SIGS.items():  # tools build only (make ab)
            fn = getattr(L, name, None)
            if fn is not None:
                fn.restype = res
                fn.argtypes = args
        if L.dsp_abi_version() != ABI_VERSION:
            raise ImportError(f"{LIB_PATH}: ABI version {L.dsp_abi_version()}, this binding needs {ABI_VERSION} "
                              "(rebuild the library)")
        _lib = L
    return _lib


def check(status: int, what: str) -> None:
    if status != DSP_OK:
        L = lib()
        raise DspError(status, what, f"{L.dsp_status_string(status).decode()}: "
                                     f"{L.dsp_last_error().decode()}")


def chan_table(ptrs) -> C.Array:
    t = (FP * max(1, len(ptrs)))()
    for i, p in enumerate(ptrs):
        t[i] = C.cast(C.c_void_p(p), FP)
    return t
