"""The oracle with AeroL's 1 s DCD timer run between messages
(tools/liboracle_tick.so: oracle/aero_oracle.cpp as it stands plus the hook
oracle_x_dcd_tick), the checker of AERO_F_DCD_TICK_BURST.

The reference's timer slot runs from the event loop, between two writeData
calls.  The model pinned here: the tick that belongs to sample 48000 k - 1
fires at the end of the message that contains that sample, after every
soft-bit group that message delivered to AeroL::Decode and before the first
group of the next message.  A message of n samples pushed after `a` samples
therefore carries (a + n) // 48000 - a // 48000 ticks."""
import ctypes

import aero_testlib as tl

FS = 48000


def _so():
    import build  # aero-cli_amd/build.py (aero_testlib puts it on the path)
    return build.build_oracletick()


class TickOracle(tl.Oracle):
    """tl.Oracle over the hooked library.  `tick=False` never calls the hook:
    the untimed model, what liboracle.so computes."""
    _libs = {}  # its own cache: tl.Oracle.lib() keeps the library under cls._libs['L']

    @classmethod
    def lib(cls):
        if 'L' not in cls._libs:
            saved = tl.ORACLE_SO
            tl.ORACLE_SO = _so()
            try:
                L = super().lib()
            finally:
                tl.ORACLE_SO = saved
            L.oracle_x_dcd_tick.argtypes = [ctypes.c_void_p]
            L.oracle_x_dcd_tick.restype = None
        return cls._libs['L']

    def __init__(self, bitrate=10500, tick=True):
        super().__init__(bitrate=bitrate, burst=True)
        self.tick = tick
        self.pushed = 0
        self.ticks = 0

    def push(self, pcm, fs=None):
        n = len(pcm)
        super().push(pcm, fs)
        k = (self.pushed + n) // FS - self.pushed // FS
        self.pushed += n
        if self.tick:
            for _ in range(k):
                self.L.oracle_x_dcd_tick(self.h)
            self.ticks += k


def messages(pcm, size):
    return [pcm[i:i + size] for i in range(0, len(pcm), size)]


def outputs(o):
    """what a burst channel delivers, in the shape the engine's accessors give it"""
    return dict(soft=o.softbits16(), hops=o.hops(), tests=o.rt_tests(), packets=o.rt_packets(),
                items=o.item_lines('A'), edges=o.events()[0])


def run(pcm, size, bitrate=10500, tick=True):
    o = TickOracle(bitrate=bitrate, tick=tick)
    for m in messages(pcm, size):
        o.push(m)
    return outputs(o)
