"""Python host mirror of the C ABI in include/aero_engine.h (ctypes).

Mirrors aero-decode's per-VFO surface: a channel is opened per ZMQ topic
(decode/decode.cpp:117-241), each ZMQ message is pushed as int16 PCM
(Decoder::audioReceived -> OqpskDemodulator::dataReceived), and ACARS items
come back in emission order (AeroL::ACARSsignal).  The library is the HIP
build in this directory; there is no CPU fallback: loading fails loudly when
the native library is missing and engine creation fails without a gfx950 GPU.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libaero_engine.so')

AERO_OK = 0
AERO_E_INVALID = -1
AERO_E_NOMEM = -2
AERO_E_HIP = -3
AERO_E_NOGPU = -4
AERO_E_FULL = -5
AERO_E_RATE = -6
AERO_E_DEVICE = -7

F_TRACE_PT = 0x1
F_TRACE_BLOCKS = 0x2
F_TIMING = 0x4
F_TRACE_SOFT = 0x8
F_TRACE_HOPS = 0x10
F_TRACE_FRAMES = 0x20
F_DCD_TICK = 0x40  # AeroL's 1 s DCD timer on the sample clock (continuous OQPSK)
F_DCD_TICK_BURST = 0x80  # the timer on burst channels: a tick at the end of the message that completes a second
F_DCD_TICK_CONT = 0x100  # the timer on continuous MSK and C channels, on the sample clock (their DCD can fall)
F_EBNO = 0x200  # continuous OQPSK / C: the reference's Eb/N0 estimate (channel_quality, pop_ebno)
F_EBNO_MSK = 0x400  # continuous MSK 600 / 1200 at any rate: MSKEbNoMeasure, with a 2 Fs ring per channel
F_TRACE_ALL =F_TRACE_PT | F_TRACE_BLOCKS | F_TRACE_SOFT | F_TRACE_HOPS | F_TRACE_FRAMES

MATH_FN = {'hypot': 0, 'atan2': 1, 'tanh': 2, 'sin': 3, 'cos': 4, 'log10': 5, 'sqrt': 6, 'fmod360': 7,
           'div': 8, 'div_c48000': 9, 'div_c360': 10, 'div_n': 11, 'div_c192000': 13, 'hypot_nr': 14, 'atan2_bf': 15,
           'tanh_bf': 16, 'sin_bf': 17, 'cos_bf': 18,
           'div_cw_wt': 19, 'set_phase_ptr': 20, 'log10_ge1': 21}
# aero_device_viterbi variants (AERO_VIT_*) and the block length of the production-source ones
VIT_VARIANT = {'wave': 0, 'regs': 1, 'regs2-self': 2, 'regs2-pair': 3, 'block4992': 4, 'block384': 5, 'block576': 6,
               'csoft': 7}
FFT_KIND = {'dit': 0, 'chain': 1}  # aero_device_fft kinds (AERO_FFT_*)
VIT_BLOCK = {'block4992': 4992, 'block384': 384, 'block576': 576, 'csoft': 5460}


class EngineCfg(ctypes.Structure):
    _fields_ = [('device', ctypes.c_int), ('max_channels', ctypes.c_int), ('flags', ctypes.c_int)]


class ChannelCfg(ctypes.Structure):
    _fields_ = [('bitrate', ctypes.c_int), ('burst', ctypes.c_int), ('fs', ctypes.c_uint32),
                ('disable_reassembly', ctypes.c_int)]


class AcarsItem(ctypes.Structure):
    _fields_ = [('aesid', ctypes.c_uint32),
                ('gesid', ctypes.c_uint8), ('qno', ctypes.c_uint8), ('refno', ctypes.c_uint8),
                ('seqno', ctypes.c_uint8),
                ('mode', ctypes.c_uint8), ('tak', ctypes.c_uint8), ('bi', ctypes.c_uint8),
                ('nonacars', ctypes.c_uint8),
                ('downlink', ctypes.c_uint8), ('valid', ctypes.c_uint8), ('hastext', ctypes.c_uint8),
                ('moretocome', ctypes.c_uint8),
                ('fragment', ctypes.c_uint8), ('label_len', ctypes.c_uint8), ('reg_len', ctypes.c_uint8),
                ('pad0', ctypes.c_uint8),
                ('label', ctypes.c_char * 4), ('reg', ctypes.c_char * 16),
                ('msg_len', ctypes.c_uint32), ('msg', ctypes.c_char * 3584)]


class ChanCfg(ctypes.Structure):
    _fields_ = [('device', ctypes.c_int), ('sample_rate', ctypes.c_int), ('center_frequency', ctypes.c_int),
                ('mix_offset', ctypes.c_int), ('correct_dc_bias', ctypes.c_int), ('max_blocks', ctypes.c_int),
                ('flags', ctypes.c_int)]


class ChanMain(ctypes.Structure):
    _fields_ = [('frequency', ctypes.c_int), ('out_rate', ctypes.c_int), ('compress_scale', ctypes.c_int),
                ('publish', ctypes.c_int)]


class ChanVfo(ctypes.Structure):
    _fields_ = [('frequency', ctypes.c_int), ('data_rate', ctypes.c_int), ('out_rate', ctypes.c_int),
                ('filter_bandwidth', ctypes.c_int), ('gain', ctypes.c_float), ('skip', ctypes.c_int)]


CHAN_F_HOST_OUT = 0x1


class ChanSurveyCfg(ctypes.Structure):
    _fields_ = [('log2n', ctypes.c_int), ('window', ctypes.c_void_p)]


class SurveyPeakCfg(ctypes.Structure):
    _fields_ = [('threshold', ctypes.c_double), ('min_bins', ctypes.c_int), ('merge_gap', ctypes.c_int)]


class SurveyPeak(ctypes.Structure):
    _fields_ = [('offset_hz', ctypes.c_double), ('bandwidth_hz', ctypes.c_double), ('ratio', ctypes.c_double),
                ('frequency', ctypes.c_longlong), ('first_bin', ctypes.c_int), ('last_bin', ctypes.c_int)]


class ChanSurveyHoldCfg(ctypes.Structure):
    _fields_ = [('group', ctypes.c_int), ('rows', ctypes.c_int), ('level', ctypes.c_void_p)]


class SurveyAct(ctypes.Structure):
    _fields_ = [('on_ratio', ctypes.c_double), ('off_ratio', ctypes.c_double), ('duty', ctypes.c_double),
                ('kind', ctypes.c_int)]


SURVEY_IDLE, SURVEY_CONTINUOUS, SURVEY_BURST = 0, 1, 2


class ChannelEvents(ctypes.Structure):
    _fields_ = [('dcd_edges', ctypes.c_int64), ('hunter_steps', ctypes.c_int64), ('hunter_fc', ctypes.c_double * 8)]


class ChannelQuality(ctypes.Structure):
    _fields_ = [('samples', ctypes.c_int64), ('ebno_db', ctypes.c_double), ('mse', ctypes.c_double),
                ('mixer_hz', ctypes.c_double), ('center_hz', ctypes.c_double), ('signal', ctypes.c_int32),
                ('ebno_valid', ctypes.c_int32)]


# every entry point declared in include/aero_engine.h and include/aero_chan.h (tests/test_abi.py checks the header)
_SIGS = {
    'aero_engine_create': (ctypes.c_int, [ctypes.POINTER(EngineCfg), ctypes.POINTER(ctypes.c_void_p)]),
    'aero_engine_destroy': (None, [ctypes.c_void_p]),
    'aero_channel_open': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ChannelCfg), ctypes.POINTER(ctypes.c_int)]),
    'aero_channel_close': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'aero_engine_reserve': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ChannelCfg), ctypes.c_int]),
    'aero_channel_export': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    'aero_channel_import': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_int)]),
    'aero_push_pcm': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.c_uint32]),
    'aero_push_pcm_batch': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                           ctypes.c_int, ctypes.c_int]),
    'aero_push_pcm_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.c_uint32]),
    'aero_run': (ctypes.c_int, [ctypes.c_void_p]),
    'aero_flush': (ctypes.c_int, [ctypes.c_void_p]),
    'aero_pop_softbits': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.POINTER(ctypes.c_size_t)]),
    'aero_pop_items': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(AcarsItem), ctypes.c_size_t,
                                      ctypes.POINTER(ctypes.c_size_t)]),
    'aero_pop_items_all': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(AcarsItem), ctypes.POINTER(ctypes.c_int),
                                          ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    'aero_pop_hops': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_size_t)]),
    'aero_trace_select': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    'aero_pop_pt': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                   ctypes.POINTER(ctypes.c_size_t)]),
    'aero_pop_blocks': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.POINTER(ctypes.c_size_t)]),
    'aero_pop_frames': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.POINTER(ctypes.c_size_t)]),
    'aero_pop_rt_tests': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.POINTER(ctypes.c_size_t)]),
    'aero_pop_c_units': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.POINTER(ctypes.c_size_t)]),
    'aero_pop_voice': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                      ctypes.POINTER(ctypes.c_size_t)]),
    'aero_pop_rt_packets': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_size_t)]),
    'aero_timing': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                   ctypes.POINTER(ctypes.c_long)]),
    'aero_timing_reset': (None, [ctypes.c_void_p]),
    'aero_samples_processed': (ctypes.c_uint64, [ctypes.c_void_p]),
    'aero_stat': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]),
    'aero_channel_stat': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p,
                                         ctypes.POINTER(ctypes.c_int64)]),
    'aero_channel_get_events': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ChannelEvents)]),
    'aero_channel_get_quality': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ChannelQuality)]),
    'aero_pop_ebno': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_size_t)]),
    'aero_sync': (ctypes.c_int, [ctypes.c_void_p]),
    'aero_device_math': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_size_t]),
    'aero_device_viterbi': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                           ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    'aero_device_fft': (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_size_t,
                                                                                 ctypes.c_void_p]),
    'aero_channel_coarse_y': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]),
    'aero_strerror': (ctypes.c_char_p, [ctypes.c_int]),
    # include/aero_chan.h
    'aero_chan_create': (ctypes.c_int, [ctypes.POINTER(ChanCfg), ctypes.POINTER(ChanMain), ctypes.c_int,
                                        ctypes.POINTER(ChanVfo), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'aero_chan_destroy': (None, [ctypes.c_void_p]),
    'aero_chan_block_len': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]),
    'aero_chan_vfo_info': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    'aero_chan_main_info': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    'aero_chan_push': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]),
    'aero_chan_run': (ctypes.c_int, [ctypes.c_void_p]),
    'aero_chan_sync': (ctypes.c_int, [ctypes.c_void_p]),
    'aero_chan_vfo_output': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(ctypes.c_size_t)]),
    'aero_chan_pop_audio': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_size_t)]),
    'aero_chan_pop_iq': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.POINTER(ctypes.c_size_t)]),
    'aero_chan_feed': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]),
    'aero_chan_vfo_open': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ChanVfo), ctypes.POINTER(ctypes.c_int)]),
    'aero_chan_vfo_close': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'aero_chan_vfo_skip': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    'aero_chan_reserve': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ChanVfo), ctypes.c_int]),
    'aero_chan_vfo_count': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]),
    'aero_chan_vfo_settle': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    'aero_chan_stat': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]),
    'aero_chan_survey_start': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ChanSurveyCfg)]),
    'aero_chan_survey_stop': (ctypes.c_int, [ctypes.c_void_p]),
    'aero_chan_survey_read': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    'aero_survey_peaks': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int,
                                         ctypes.POINTER(SurveyPeakCfg), ctypes.POINTER(SurveyPeak), ctypes.c_size_t,
                                         ctypes.POINTER(ctypes.c_size_t)]),
    'aero_chan_survey_hold_start': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ChanSurveyHoldCfg)]),
    'aero_chan_survey_hold_stop': (ctypes.c_int, [ctypes.c_void_p]),
    'aero_chan_survey_hold_read': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    'aero_chan_survey_hold_rows': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                  ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t)]),
    'aero_survey_activity': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                            ctypes.POINTER(SurveyPeak), ctypes.c_size_t, ctypes.POINTER(SurveyAct)]),
}

_lib = None


def _torch_hip_runtime():
    """Paths of the HIP/HSA runtime copies a PyTorch-ROCm wheel bundles
    (torch/lib), or [] when torch is not installed.  Found without importing
    torch (no HIP initialisation happens here)."""
    import importlib.util
    spec = importlib.util.find_spec('torch')
    if spec is None or not spec.origin:
        return []
    tlib = os.path.join(os.path.dirname(spec.origin), 'lib')
    return [p for p in (os.path.join(tlib, 'libhsa-runtime64.so'), os.path.join(tlib, 'libamdhip64.so'))
            if os.path.exists(p)]


def load_library(path=None):
    """Loads libaero_engine.so (or $AERO_ENGINE_SO, an experimental build of
    the same sources); raises when the HIP build is missing.

    One HIP runtime per process: the PyTorch-ROCm wheel bundles its own
    libamdhip64 / libhsa-runtime64 (SONAME libamdhip64.so.7, the same as
    /opt/rocm's, which the engine links).  Loaded after torch, the engine
    binds to torch's copy by SONAME; loaded first, it would pull in
    /opt/rocm's copy and torch would then load a second runtime from
    torch/lib, and a device pointer allocated by one runtime is unknown to
    the other (aero_push_pcm_dev / aero_chan_push(dev) fail).  So torch's
    copy, when torch is installed, is loaded first by its absolute path:
    torch's later load of the same file reuses it (same inode) and the engine
    binds to it by SONAME, in either import order.  Without torch (the C++
    host) the engine uses /opt/rocm's runtime."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get('AERO_ENGINE_SO') or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError('libaero_engine.so not built (%s); run aero-cli_amd/build.py' % path)
    for rt in _torch_hip_runtime():
        ctypes.CDLL(rt, mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if path == LIB_PATH:
                raise
            continue  # an older experimental build (A/B) without a newer entry point
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class AeroError(RuntimeError):
    def __init__(self, rc, what):
        lib = load_library()
        super().__init__('%s failed: %s (%d)' % (what, lib.aero_strerror(rc).decode(), rc))
        self.rc = rc


def _check(rc, what):
    if rc != AERO_OK:
        raise AeroError(rc, what)


def item_line(it):
    """Canonical text of one ACARSItem, identical to the oracle's emit_item."""
    def hx(b):
        return b.hex()
    kind = 'F' if it.fragment else 'A'
    head = ('%s aes=%06X ges=%02X qno=%02X refno=%02X mode=%02X tak=%02X bi=%02X '
            'nonacars=%d downlink=%d valid=%d hastext=%d more=%d' % (
                kind, it.aesid, it.gesid, it.qno, it.refno, it.mode, it.tak, it.bi, it.nonacars,
                it.downlink, it.valid, it.hastext, it.moretocome))
    label = bytes(it.label)[:it.label_len]
    reg = bytes(it.reg)[:it.reg_len]
    msg = ctypes.string_at(ctypes.addressof(it) + AcarsItem.msg.offset, it.msg_len)
    return head + ' label=' + hx(label) + ' reg=' + hx(reg) + ' msg=' + hx(msg)


def blob_kinds(blob):
    """(bitrate, burst, fs, disable_reassembly) of every blob of an exported
    batch (the header fields of include/aero_engine.h; lengths checked)."""
    import struct
    out, pos = [], 0
    while pos + 48 <= len(blob):
        bitrate, burst, fs, dis = struct.unpack_from('<iiIi', blob, pos + 12)
        total, = struct.unpack_from('<Q', blob, pos + 40)
        if total < 64 or pos + total > len(blob):
            break
        out.append((bitrate, burst, fs, dis))
        pos += total
    return out


class Engine:
    """Batched MI355X Aero demodulator (one engine per GPU)."""

    def __init__(self, max_channels, device=0, flags=0):
        self.lib = load_library()
        cfg = EngineCfg(device, max_channels, flags)
        h = ctypes.c_void_p()
        _check(self.lib.aero_engine_create(ctypes.byref(cfg), ctypes.byref(h)), 'aero_engine_create')
        self.h = h
        self.flags = flags
        self._fs = {}

    def close(self):
        if self.h:
            self.lib.aero_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # sample rate aero-decode feeds each bit rate (decode/decode.cpp:142-159)
    RATE = {10500: 48000, 600: 12000, 1200: 24000, 8400: 48000}

    def open_channel(self, bitrate=10500, fs=None, disable_reassembly=False, burst=False):
        fs = fs or self.RATE.get(bitrate, 48000)
        cfg = ChannelCfg(bitrate, int(burst), fs, int(disable_reassembly))
        ch = ctypes.c_int()
        _check(self.lib.aero_channel_open(self.h, ctypes.byref(cfg), ctypes.byref(ch)), 'aero_channel_open')
        self._fs[ch.value] = fs
        return ch.value

    def close_channel(self, ch):
        """aero_channel_close: drops the channel's pending samples and
        undelivered outputs; its id and slot go to the next open_channel."""
        _check(self.lib.aero_channel_close(self.h, ch), 'aero_channel_close')
        self._fs.pop(ch, None)

    def export_channels(self, chans):
        """aero_channel_export: a snapshot of the channels' decoder state, one
        blob per channel back to back; the channels stay open."""
        chans = list(chans)
        arr = (ctypes.c_int * max(1, len(chans)))(*chans)
        need = ctypes.c_size_t()
        _check(self.lib.aero_channel_export(self.h, arr, len(chans), None, 0, ctypes.byref(need)),
               'aero_channel_export')
        buf = np.empty(max(1, need.value), dtype=np.uint8)
        _check(self.lib.aero_channel_export(self.h, arr, len(chans), buf.ctypes.data, need.value,
                                            ctypes.byref(need)), 'aero_channel_export')
        return buf[:need.value].tobytes()

    def export_channel(self, ch):
        return self.export_channels([ch])

    def import_channels(self, blob):
        """aero_channel_import: opens one channel per blob with the exported
        state; returns their ids (all of the batch or, on an error, none)."""
        src = np.frombuffer(blob, dtype=np.uint8)
        # a blob is at least its 64 bytes of header and section lengths
        cap = max(1, len(src) // 64)
        out = (ctypes.c_int * cap)()
        n = ctypes.c_int()
        _check(self.lib.aero_channel_import(self.h, src.ctypes.data if len(src) else None, len(src), out, cap,
                                            ctypes.byref(n)), 'aero_channel_import')
        chans = [out[i] for i in range(n.value)]
        kinds = blob_kinds(blob)
        for ch, (bitrate, burst, fs, dis) in zip(chans, kinds):
            self._fs[ch] = fs
        return chans

    def import_channel(self, blob):
        chans = self.import_channels(blob)
        if len(chans) != 1:
            for ch in chans:
                self.close_channel(ch)
            raise ValueError('import_channel: %d blobs' % len(chans))
        return chans[0]

    def reserve(self, n, bitrate=10500, fs=None, burst=False):
        """aero_engine_reserve: the kind's group is created with n slots
        instead of max_channels (before the kind's first open_channel)."""
        fs = fs or self.RATE.get(bitrate, 48000)
        cfg = ChannelCfg(bitrate, int(burst), fs, 0)
        _check(self.lib.aero_engine_reserve(self.h, ctypes.byref(cfg), n), 'aero_engine_reserve')

    def push(self, ch, pcm, fs=None):
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        fs = fs or self._fs.get(ch, 48000)
        _check(self.lib.aero_push_pcm(self.h, ch, pcm.ctypes.data, pcm.size, fs), 'aero_push_pcm')

    def push_batch(self, pcm, nch=None):
        """pcm: int16 [n, ld] host array (time-major) for channels 0..nch-1."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        n, ld = pcm.shape
        _check(self.lib.aero_push_pcm_batch(self.h, pcm.ctypes.data, n, ld, nch or ld, 0), 'aero_push_pcm_batch')

    def push_device(self, ch, ptr, n, fs=None):
        """ptr: HIP device pointer of n int16 samples for channel ch."""
        fs = fs or self._fs.get(ch, 48000)
        _check(self.lib.aero_push_pcm_dev(self.h, ch, ctypes.c_void_p(ptr), n, fs), 'aero_push_pcm_dev')

    def push_batch_host(self, ptr, n, ld, nch):
        """ptr: host pointer of int16 [n, ld]; pinned memory (e.g. a torch
        pin_memory() tensor) is DMA'd straight into HBM."""
        _check(self.lib.aero_push_pcm_batch(self.h, ctypes.c_void_p(ptr), n, ld, nch, 0), 'aero_push_pcm_batch')

    def push_batch_device(self, ptr, n, ld, nch):
        """ptr: HIP device pointer of int16 [n, ld] (e.g. torch tensor.data_ptr())."""
        _check(self.lib.aero_push_pcm_batch(self.h, ctypes.c_void_p(ptr), n, ld, nch, 1), 'aero_push_pcm_batch')

    def trace_select(self, channels):
        """Keeps traces (soft bits, hops, pt, blocks, frames) of these
        continuous channels only; [] keeps every channel's again."""
        arr = (ctypes.c_int * max(1, len(channels)))(*[int(c) for c in channels])
        _check(self.lib.aero_trace_select(self.h, arr, len(channels)), 'aero_trace_select')

    def run(self):
        _check(self.lib.aero_run(self.h), 'aero_run')

    def flush(self):
        _check(self.lib.aero_flush(self.h), 'aero_flush')

    def sync(self):
        _check(self.lib.aero_sync(self.h), 'aero_sync')

    def _pop(self, fn, ch, dtype, rec=1):
        out = []
        cap = 1 << 20
        while True:
            buf = np.empty(cap * rec, dtype=dtype)
            n = ctypes.c_size_t()
            _check(fn(self.h, ch, buf.ctypes.data, cap, ctypes.byref(n)), fn.__name__)
            out.append(buf[:n.value * rec].copy())
            if n.value < cap:
                break
        r = np.concatenate(out)
        return r.reshape(-1, rec) if rec > 1 else r

    def softbits(self, ch):
        return self._pop(self.lib.aero_pop_softbits, ch, np.int16).astype(np.uint8)

    def softbits16(self, ch):
        """burst channels: delivered soft bits with -1 start-of-packet markers"""
        return self._pop(self.lib.aero_pop_softbits, ch, np.int16)

    def rt_tests(self, ch):
        """burst channels: (blockptr, result code) of every R/T test"""
        return self._pop(self.lib.aero_pop_rt_tests, ch, np.uint8).view(np.uint32).reshape(-1, 2)

    def rt_packets(self, ch):
        """burst channels: [(kind 'R'/'T', infofield bytes)] of every decoded R/T packet"""
        raw = self._pop(self.lib.aero_pop_rt_packets, ch, np.uint8)
        out, i = [], 0
        while i < len(raw):
            kind, ln = np.frombuffer(raw[i:i + 8].tobytes(), np.uint32)
            out.append((chr(kind), bytes(raw[i + 8:i + 8 + int(ln)])))
            i += 8 + int(ln)
        return out

    def c_units(self, ch):
        """C channel: every CRC-valid Call_progress SU, [n, 12] bytes"""
        return self._pop(self.lib.aero_pop_c_units, ch, np.uint8, 12)

    def voice(self, ch):
        """C channel: per frame (AES of its last Call_progress, 300 voice bytes)"""
        raw = self._pop(self.lib.aero_pop_voice, ch, np.uint8, 304)
        return [(int(np.frombuffer(r[:4].tobytes(), np.uint32)[0]), bytes(r[4:])) for r in raw]

    def hops(self, ch):
        return self._pop(self.lib.aero_pop_hops, ch, np.float64, 6)

    def pt(self, ch):
        return self._pop(self.lib.aero_pop_pt, ch, np.float64, 2)

    def blocks(self, ch):
        return self._pop(self.lib.aero_pop_blocks, ch, np.uint8)

    def frames(self, ch):
        return self._pop(self.lib.aero_pop_frames, ch, np.uint8)

    def items(self, ch):
        out = []
        arr = (AcarsItem * 64)()
        while True:
            n = ctypes.c_size_t()
            _check(self.lib.aero_pop_items(self.h, ch, arr, 64, ctypes.byref(n)), 'aero_pop_items')
            out.extend(item_line(arr[i]) for i in range(n.value))
            if n.value < 64:
                return out

    def drain_items(self, lines=False, cap=4096, keep=None):
        """Pops the items of every channel (aero_pop_items_all).  Returns the
        count, or (channel, canonical line) pairs with lines=True (only the
        channels in the set `keep`, when given)."""
        if getattr(self, '_drain_cap', 0) != cap:
            self._drain_buf = ((AcarsItem * cap)(), (ctypes.c_int * cap)())
            self._drain_cap = cap
        arr, chs = self._drain_buf
        total, out = 0, []
        while True:
            n = ctypes.c_size_t()
            _check(self.lib.aero_pop_items_all(self.h, arr, chs, cap, ctypes.byref(n)), 'aero_pop_items_all')
            total += n.value
            if lines:
                out.extend((chs[i], item_line(arr[i])) for i in range(n.value) if keep is None or chs[i] in keep)
            if n.value < cap:
                return out if lines else total

    def timing(self, name):
        ms = ctypes.c_double()
        k = ctypes.c_long()
        _check(self.lib.aero_timing(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(k)), 'aero_timing')
        return ms.value, k.value

    def timing_reset(self):
        self.lib.aero_timing_reset(self.h)

    def stat(self, name):
        """aero_stat counter: 'viterbi_jobs', 'frames', 'su_crc_ok' (and burst 'rt_*'), or the
        continuous groups' 'device_bytes' / 'groups', 'slot_resets' (reset-kernel launches),
        'slot_copies' (pack / unpack launches of export_channels / import_channels) or
        'ebno_launches' (launches of the Eb/N0 kernels, F_EBNO / F_EBNO_MSK)."""
        v = ctypes.c_uint64()
        _check(self.lib.aero_stat(self.h, name.encode(), ctypes.byref(v)), 'aero_stat')
        return int(v.value)

    def channel_stat(self, ch, name):
        """aero_channel_stat: 'hunter_scans' or 'freq_center'."""
        v = ctypes.c_int64()
        _check(self.lib.aero_channel_stat(self.h, ch, name.encode(), ctypes.byref(v)), 'aero_channel_stat')
        return int(v.value)

    def channel_events(self, ch):
        """aero_channel_get_events: (dcd_edges, hunter_steps, [centre of each
        of the last min(8, steps) steps, oldest first])."""
        ev = ChannelEvents()
        _check(self.lib.aero_channel_get_events(self.h, ch, ctypes.byref(ev)), 'aero_channel_get_events')
        n = int(ev.hunter_steps)
        fcs = [ev.hunter_fc[(k - 1) & 7] for k in range(max(1, n - 7), n + 1)]
        return int(ev.dcd_edges), n, fcs

    def channel_quality(self, ch):
        """aero_channel_get_quality: dict of samples, ebno_db, mse, mixer_hz, center_hz, signal,
        ebno_valid (ebno_db only with F_EBNO on a continuous OQPSK or C channel, 0 .. 50 dB, or with
        F_EBNO_MSK on a continuous MSK channel, (-inf, 50] dB and negative during the first 2 s)."""
        q = ChannelQuality()
        _check(self.lib.aero_channel_get_quality(self.h, ch, ctypes.byref(q)), 'aero_channel_get_quality')
        return dict(samples=int(q.samples), ebno_db=q.ebno_db, mse=q.mse, mixer_hz=q.mixer_hz,
                    center_hz=q.center_hz, signal=int(q.signal), ebno_valid=int(q.ebno_valid))

    def ebno(self, ch):
        """aero_pop_ebno: [n, 2] (sample index, EbNo) per hop boundary reached (F_TRACE_HOPS with F_EBNO,
        or with F_EBNO_MSK on a continuous MSK channel)."""
        return self._pop(self.lib.aero_pop_ebno, ch, np.float64, 2)

    def samples_processed(self):
        return int(self.lib.aero_samples_processed(self.h))

    def device_math(self, fn, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x) if y is None else np.ascontiguousarray(y, dtype=np.float64)
        out = np.empty_like(x)
        _check(self.lib.aero_device_math(self.h, MATH_FN[fn], x.ctypes.data, y.ctypes.data, out.ctypes.data,
                                         x.size), 'aero_device_math')
        return out

    def device_viterbi(self, variant, rows, nsoft=None):
        """aero_device_viterbi (diagnostic): decodes the rows of a 2-D uint8
        array with one of the device Viterbi decoders.  Flat variants: rows
        are codewords, returns bits [ncw, nsoft / 2].  Production-source
        variants: rows are records (block, 62 overlap bytes, first, pad) and
        nsoft the stream length; returns (bits, overlap [ncw, 62])."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        assert rows.ndim == 2
        src = variant in VIT_BLOCK
        nsoft = rows.shape[1] if nsoft is None else int(nsoft)
        bits = np.zeros((rows.shape[0], nsoft // 2), dtype=np.uint8)
        ov = np.zeros((rows.shape[0], 62), dtype=np.uint8)
        _check(self.lib.aero_device_viterbi(self.h, VIT_VARIANT[variant], rows.ctypes.data, rows.shape[0], nsoft,
                                            bits.ctypes.data, ov.ctypes.data if src else None),
               'aero_device_viterbi')
        return (bits, ov) if src else bits

    def device_fft(self, kind, records, inverse=False, depth=0, start=1, stop=0):
        """aero_device_fft (diagnostic): the rows of a 2-D complex128 array
        (4096, 8192 or 16384 values, natural order) through the device's
        'dit' transform (inverse: the sum without 1/N) or the coarse
        estimator's 'chain' at depth 1-3 with the bins start..stop zeroed
        after the first transform; returns the transforms, natural order."""
        records = np.ascontiguousarray(records, dtype=np.complex128)
        assert records.ndim == 2
        n = records.shape[1]
        log2n = n.bit_length() - 1 if n > 0 and n & (n - 1) == 0 else 0
        out = np.empty_like(records)
        _check(self.lib.aero_device_fft(self.h, FFT_KIND.get(kind, -1), log2n, int(inverse), int(depth), int(start),
                                        int(stop), records.ctypes.data, records.shape[0], out.ctypes.data),
               'aero_device_fft')
        return out

    def channel_coarse_y(self, ch):
        """aero_channel_coarse_y: (first_bin, y[first_bin : first_bin + n]) of
        the coarse estimator's smoothed spectrum as the next hop reads it."""
        y = np.empty(16384, dtype=np.float64)
        n, first = ctypes.c_size_t(), ctypes.c_int()
        _check(self.lib.aero_channel_coarse_y(self.h, ch, y.ctypes.data, y.size, ctypes.byref(n), ctypes.byref(first)),
               'aero_channel_coarse_y')
        return int(first.value), y[:n.value].copy()


# ------------------------------------------------------------------ channeliser
def vfo_out_rate(data_rate, out_rate=0):
    """[vfos] out_rate default by data_rate (publish/publisher.cpp:164-176)."""
    if out_rate or not data_rate:
        return out_rate
    return {600: 12000, 1200: 24000}.get(int(data_rate), 48000)


def vfo_bitrate(data_rate):
    """aero-decode bit rate of a [vfos] entry's audio (10500 unless 600/1200)."""
    return int(data_rate) if int(data_rate) in (600, 1200) else 10500


def parse_sdr_ini(text):
    """SDRReceiver INI as QSettings reads it for aero-publish
    (publish/publisher.cpp:55-227): returns (general, mains, vfos) dicts with
    the keys the publisher uses; arrays are QSettings' [name] size=N,
    i\\key=value entries."""
    sections, cur = {}, 'General'
    for raw in text.splitlines():
        line = raw.strip()
        if not line or line[0] in ';#':
            continue
        if line.startswith('[') and line.endswith(']'):
            cur = line[1:-1]
            continue
        if '=' in line:
            k, v = line.split('=', 1)
            sections.setdefault(cur, {})[k.strip()] = v.strip()

    def to_int(v):  # QVariant::toInt: 0 when the text is not an integer
        try:
            return int(v)
        except (TypeError, ValueError):
            return 0

    def to_float(v):
        try:
            return float(v)
        except (TypeError, ValueError):
            return 0.0

    def array(name):
        sec = sections.get(name, {})
        out = []
        for i in range(1, to_int(sec.get('size')) + 1):
            pre = '%d\\' % i
            out.append({k[len(pre):]: v for k, v in sec.items() if k.startswith(pre)})
        return out

    g = sections.get('General', {})
    general = dict(sample_rate=to_int(g.get('sample_rate')), center_frequency=to_int(g.get('center_frequency')),
                   mix_offset=to_int(g.get('mix_offset')), correct_dc_bias=g.get('correct_dc_bias') == '1',
                   zmq_address=g.get('zmq_address', ''))
    mains = [dict(frequency=to_int(d.get('frequency')), out_rate=to_int(d.get('out_rate')),
                  compress_scale=to_int(d.get('compress_scale')),
                  publish=int(bool(d.get('zmq_address')) and bool(d.get('zmq_topic'))))
             for d in array('main_vfos')]
    vfos = [dict(frequency=to_int(d.get('frequency')), data_rate=to_int(d.get('data_rate')),
                 out_rate=to_int(d.get('out_rate')), filter_bandwidth=to_int(d.get('filter_bandwidth')),
                 gain=to_float(d.get('gain')), topic=d.get('topic', ''))
            for d in array('vfos')]
    return general, mains, vfos


class Channeliser:
    """aero-publish's channeliser on one GPU (include/aero_chan.h):
    Publisher::loadSettings + demodData (publish/publisher.cpp:55-306) and
    vfo::process (publish/vfo.cpp:154-313).  `mains` / `vfos` are the INI's
    [main_vfos] / [vfos] entries (dicts as parse_sdr_ini returns); `skip`
    marks [vfos] entries another process computes."""

    def __init__(self, sample_rate, center_frequency, mains, vfos, mix_offset=0, correct_dc_bias=False,
                 max_blocks=8, device=0, host_out=False, skip=None):
        self.lib = load_library()
        cfg = ChanCfg(device, int(sample_rate), int(center_frequency), int(mix_offset), int(bool(correct_dc_bias)),
                      int(max_blocks), CHAN_F_HOST_OUT if host_out else 0)
        m = (ChanMain * max(1, len(mains)))()
        for i, d in enumerate(mains):
            m[i] = ChanMain(int(d['frequency']), int(d.get('out_rate', 0)), int(d.get('compress_scale', 0)),
                            int(d.get('publish', 0)))
        v = (ChanVfo * max(1, len(vfos)))()
        for i, d in enumerate(vfos):
            v[i] = self._vfo(d, skip[i] if skip is not None else False)
        h = ctypes.c_void_p()
        _check(self.lib.aero_chan_create(ctypes.byref(cfg), m, len(mains), v, len(vfos), ctypes.byref(h)),
               'aero_chan_create')
        self.h = h
        self.nmain, self.nvfo = len(mains), len(vfos)
        b = ctypes.c_int()
        _check(self.lib.aero_chan_block_len(h, ctypes.byref(b)), 'aero_chan_block_len')
        self.block_len = b.value

    def close(self):
        if self.h:
            self.lib.aero_chan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def vfo_info(self, v):
        i = (ctypes.c_int * 5)()
        _check(self.lib.aero_chan_vfo_info(self.h, v, i), 'aero_chan_vfo_info')
        return dict(main=i[0], out_rate=i[1], samples_per_block=i[2], halfbands=i[3], late=i[4])

    def main_info(self, m):
        i = (ctypes.c_int * 3)()
        _check(self.lib.aero_chan_main_info(self.h, m, i), 'aero_chan_main_info')
        return dict(out_rate=i[0], samples_per_block=i[1], halfbands=i[2])

    def push(self, iq):
        """iq: complex64 host samples, whole reads of block_len."""
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        nb = iq.size // self.block_len
        if nb * self.block_len != iq.size:
            raise ValueError('push whole reads of %d samples' % self.block_len)
        _check(self.lib.aero_chan_push(self.h, iq.ctypes.data, nb, 0), 'aero_chan_push')

    def push_device(self, ptr, nblocks):
        """ptr: HIP device pointer of nblocks * block_len interleaved CF32 samples."""
        _check(self.lib.aero_chan_push(self.h, ctypes.c_void_p(ptr), nblocks, 1), 'aero_chan_push')

    def run(self):
        _check(self.lib.aero_chan_run(self.h), 'aero_chan_run')

    def sync(self):
        _check(self.lib.aero_chan_sync(self.h), 'aero_chan_sync')

    def output_device(self, v):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(self.lib.aero_chan_vfo_output(self.h, v, ctypes.byref(p), ctypes.byref(n)), 'aero_chan_vfo_output')
        return p.value, n.value

    def _pop(self, fn, i, dtype):
        out, cap = [], 1 << 20
        while True:
            buf = np.empty(cap, dtype=dtype)
            n = ctypes.c_size_t()
            _check(fn(self.h, i, buf.ctypes.data, cap, ctypes.byref(n)), fn.__name__)
            out.append(buf[:n.value].copy())
            if n.value < cap:
                return np.concatenate(out)

    def audio(self, v):
        return self._pop(self.lib.aero_chan_pop_audio, v, np.int16)

    def iq(self, m):
        return self._pop(self.lib.aero_chan_pop_iq, m, np.int8)

    def feed(self, engine, channels):
        """channels[v]: engine channel of [vfos] entry v, or -1; vfo_count() entries."""
        n = self.vfo_count()
        if len(channels) < n:
            raise ValueError('feed needs one channel (or -1) for each of the %d [vfos] ids' % n)
        arr = (ctypes.c_int * max(1, n))(*[int(c) for c in channels[:n]])
        _check(self.lib.aero_chan_feed(self.h, engine.h, arr), 'aero_chan_feed')

    # ---- [vfos] entries while the receiver runs (include/aero_chan.h)
    @staticmethod
    def _vfo(d, skip=False):
        return ChanVfo(int(d['frequency']), int(d.get('data_rate', 0)), int(d.get('out_rate', 0)),
                       int(d.get('filter_bandwidth', 0)), float(d.get('gain', 0.0)), int(bool(skip)))

    def open_vfo(self, vfo, skip=False):
        """Adds the [vfos] entry `vfo` (a dict as in the constructor); returns its id, the smallest
        free one.  It takes part from the next read pushed, with zero filter histories and the NCO
        phase of the reads taken so far: after settle(id) samples its audio is that of an entry that
        was always there.  Reads pushed and not yet run are run first."""
        v = ctypes.c_int()
        _check(self.lib.aero_chan_vfo_open(self.h, ctypes.byref(self._vfo(vfo, skip)), ctypes.byref(v)),
               'aero_chan_vfo_open')
        return v.value

    def close_vfo(self, v):
        """Removes entry v; its slot is reused by the next start of the same shape."""
        _check(self.lib.aero_chan_vfo_close(self.h, v), 'aero_chan_vfo_close')

    def skip_vfo(self, v, skip=True):
        """Sets or clears entry v's skip flag (another process computes it); the id stays."""
        _check(self.lib.aero_chan_vfo_skip(self.h, v, int(bool(skip))), 'aero_chan_vfo_skip')

    def reserve(self, like, n):
        """Pre-allocates n free slots of the shape the entry `like` resolves to."""
        _check(self.lib.aero_chan_reserve(self.h, ctypes.byref(self._vfo(like)), int(n)), 'aero_chan_reserve')

    def vfo_count(self):
        """One past the largest [vfos] id in use: the length feed() expects."""
        n = ctypes.c_int()
        _check(self.lib.aero_chan_vfo_count(self.h, ctypes.byref(n)), 'aero_chan_vfo_count')
        return n.value

    def settle(self, v):
        """Output samples after a start within which entry v may differ from one that was always there."""
        n = ctypes.c_size_t()
        _check(self.lib.aero_chan_vfo_settle(self.h, v, ctypes.byref(n)), 'aero_chan_vfo_settle')
        return int(n.value)

    def stat(self, name):
        """aero_chan_stat: 'device_bytes', 'vfo_inits' (start-kernel launches), 'slots_free',
        'survey_launches', 'survey_segments' or 'survey_groups'."""
        v = ctypes.c_uint64()
        _check(self.lib.aero_chan_stat(self.h, name.encode(), ctypes.byref(v)), 'aero_chan_stat')
        return int(v.value)

    # ---- wideband carrier survey (include/aero_chan.h)
    def survey_start(self, log2n, window=None):
        """Starts the averaged power spectrum of the input on segments of 2**log2n samples (12, 13
        or 14), from the next read pushed.  window: None, 2**log2n float64 values, or 'hann'
        (0.5 - 0.5 cos(2 pi i / N), built with numpy: a convenience, nothing exact rests on it)."""
        n = 1 << int(log2n)
        if isinstance(window, str):
            if window != 'hann':
                raise ValueError('unknown window %r' % window)
            window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)
        if window is not None:
            window = np.ascontiguousarray(window, dtype=np.float64)
            if window.shape != (n,):
                raise ValueError('the window holds %d values' % n)
        cfg = ChanSurveyCfg(int(log2n), window.ctypes.data if window is not None else None)
        _check(self.lib.aero_chan_survey_start(self.h, ctypes.byref(cfg)), 'aero_chan_survey_start')
        self._survey_n = n

    def survey_stop(self):
        _check(self.lib.aero_chan_survey_stop(self.h), 'aero_chan_survey_stop')

    def survey_read(self, reset=False):
        """(summed power per bin as float64[N], natural bin order; segments summed), after the runs
        launched so far; reset=True then zeroes both (the segment grid goes on)."""
        out = np.zeros(getattr(self, '_survey_n', 1 << 14), dtype=np.float64)
        seg = ctypes.c_uint64()
        _check(self.lib.aero_chan_survey_read(self.h, out.ctypes.data, out.size, ctypes.byref(seg), int(bool(reset))),
               'aero_chan_survey_read')
        return out, int(seg.value)

    # ---- peak / min hold, duty and waterfall beside the survey
    def survey_hold_start(self, group, rows=0, level=None):
        """Starts a hold beside the survey that is on: groups of `group` consecutive segments from
        the next segment completed; per bin the largest and smallest group sum, with `level`
        (float64[N], natural bin order) the number of group sums above it, and with rows > 0 a
        ring of the last `rows` group sums."""
        n = getattr(self, '_survey_n', 0)
        if level is not None:
            level = np.ascontiguousarray(level, dtype=np.float64)
            if level.shape != (n,):
                raise ValueError('the level holds %d values' % n)
        cfg = ChanSurveyHoldCfg(int(group), int(rows), level.ctypes.data if level is not None else None)
        _check(self.lib.aero_chan_survey_hold_start(self.h, ctypes.byref(cfg)), 'aero_chan_survey_hold_start')
        self._hold_rows = int(rows)

    def survey_hold_stop(self):
        _check(self.lib.aero_chan_survey_hold_stop(self.h), 'aero_chan_survey_hold_stop')

    def survey_hold_read(self, reset=False):
        """(peak float64[N], low float64[N], busy uint32[N], groups) after the runs launched so far;
        reset=True then sets them back to +0, +inf, 0 and 0 (the unfinished group goes on)."""
        n = getattr(self, '_survey_n', 1 << 14)
        peak, low, busy = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint32)
        g = ctypes.c_uint64()
        _check(self.lib.aero_chan_survey_hold_read(self.h, peak.ctypes.data, low.ctypes.data, busy.ctypes.data, n,
                                                   ctypes.byref(g), int(bool(reset))), 'aero_chan_survey_hold_read')
        return peak, low, busy, int(g.value)

    def survey_hold_rows(self, cap_rows=None):
        """(the last group sums as float64[n][N], oldest first; the first one's group index).  A
        cap_rows below the rows held returns the newest cap_rows (AERO_E_FULL is not an error here)."""
        n = getattr(self, '_survey_n', 1 << 14)
        cap = getattr(self, '_hold_rows', 0) if cap_rows is None else int(cap_rows)
        out = np.zeros((max(cap, 1), n), dtype=np.float64)
        first, got = ctypes.c_uint64(), ctypes.c_size_t()
        rc = self.lib.aero_chan_survey_hold_rows(self.h, out.ctypes.data, cap, ctypes.byref(first), ctypes.byref(got))
        if rc not in (AERO_OK, AERO_E_FULL):
            raise AeroError(rc, 'aero_chan_survey_hold_rows')
        self.hold_rows_full = rc == AERO_E_FULL
        return out[:got.value], int(first.value)


def survey_peaks(power, log2n, sample_rate, center, mix_offset=0, threshold=8.0, min_bins=2, merge_gap=2):
    """aero_survey_peaks (host only, no GPU): the carriers in a survey spectrum as dicts with
    offset_hz, bandwidth_hz, ratio, frequency (what a [vfos] entry's frequency takes to be centred
    on the carrier), first_bin and last_bin, in ascending frequency."""
    lib = load_library()
    power = np.ascontiguousarray(power, dtype=np.float64)
    if power.shape != (1 << int(log2n),):
        raise ValueError('the spectrum holds %d values' % (1 << int(log2n)))
    cfg = SurveyPeakCfg(float(threshold), int(min_bins), int(merge_gap))
    n = ctypes.c_size_t()
    args = (power.ctypes.data, int(log2n), int(sample_rate), int(center), int(mix_offset), ctypes.byref(cfg))
    rc = lib.aero_survey_peaks(*args, None, 0, ctypes.byref(n))
    if rc not in (AERO_OK, AERO_E_FULL):
        raise AeroError(rc, 'aero_survey_peaks')
    out = (SurveyPeak * max(1, n.value))()
    _check(lib.aero_survey_peaks(*args, out, n.value, ctypes.byref(n)), 'aero_survey_peaks')
    return [dict(offset_hz=p.offset_hz, bandwidth_hz=p.bandwidth_hz, ratio=p.ratio, frequency=int(p.frequency),
                 first_bin=p.first_bin, last_bin=p.last_bin) for p in out[:n.value]]


def survey_activity(power, segments, peak, low, busy, groups, group, log2n, threshold, runs):
    """aero_survey_activity (host only, no GPU): per run of survey_peaks (dicts with first_bin and
    last_bin) a dict with on_ratio, off_ratio, duty (-1.0 when busy is None) and kind (SURVEY_IDLE,
    SURVEY_CONTINUOUS or SURVEY_BURST)."""
    lib = load_library()
    n = 1 << int(log2n) if 0 <= int(log2n) <= 30 else 0
    arr = []
    for a, t in ((power, np.float64), (peak, np.float64), (low, np.float64), (busy, np.uint32)):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=t)
            if 2 <= int(log2n) <= 24 and a.shape != (n,):
                raise ValueError('the arrays hold %d values' % n)
        arr.append(a)
    pk = (SurveyPeak * max(1, len(runs)))()
    for p, r in zip(pk, runs):
        p.first_bin, p.last_bin = int(r['first_bin']), int(r['last_bin'])
    out = (SurveyAct * max(1, len(runs)))()
    _check(lib.aero_survey_activity(arr[0].ctypes.data, int(segments), arr[1].ctypes.data, arr[2].ctypes.data,
                                    arr[3].ctypes.data if arr[3] is not None else None, int(groups), int(group),
                                    int(log2n), float(threshold), pk, len(runs), out), 'aero_survey_activity')
    return [dict(on_ratio=o.on_ratio, off_ratio=o.off_ratio, duty=o.duty, kind=o.kind) for o in out[:len(runs)]]
