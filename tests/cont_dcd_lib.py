"""The model of AERO_F_DCD_TICK_CONT (AeroL's 1 s DCD timer on continuous
600/1200-bps MSK channels and the 8400-bps C channel) and its checkers.

The timer runs on the sample clock.  A channel counts the samples until its
next tick, starting at the rate Fs it was opened at; the tick fires after the
sample that takes the count to 0 (after everything that sample delivered to
AeroL::Decode / DecodeC, before anything the next one delivers) and the count
restarts at the current Fs.  An MSK rate change Fs_old -> Fs_new between two
messages rescales the elapsed part of the second in integers:

    elapsed = Fs_old - left;  left = Fs_new - (elapsed * Fs_new) // Fs_old

MSK checker: the oracle's MSK path is chunk-invariant, so the hooked library
of tests/oracle_tick.py (oracle_x_dcd_tick, callable between two messages) is
fed the stream cut additionally at the model's tick samples.
C checker: the C channel's output depends on its message boundaries, which
therefore stay; its rule is "after sample n with (n + 1) % 48000 == 0", what
the oracle itself does at 8400 bps with dcd_tick=True."""
import functools

import numpy as np

import aero_testlib as tl
from oracle_tick import TickOracle

C_FS = 48000


def rescale(left, fs_old, fs_new):
    """samples until the next tick after a rate change"""
    elapsed = fs_old - left
    return fs_new - (elapsed * fs_new) // fs_old


class TickClock:
    """the samples-until-next-tick count of one channel"""

    def __init__(self, fs, rule='rescale'):
        """rule: what a rate change does to the running second.  'rescale' is the
        model; 'restart' (a new second begins) is a wrong rule, kept so that a
        test can show that its stream tells the two apart"""
        self.fs = int(fs)
        self.left = int(fs)
        self.ticks = 0
        self.rule = rule

    def set_rate(self, fs):
        fs = int(fs)
        if fs != self.fs:
            self.left = rescale(self.left, self.fs, fs) if self.rule == 'rescale' else fs
            self.fs = fs

    def cuts(self, n):
        """offsets in (0, n] of a message of n samples after which a tick fires"""
        out, p = [], 0
        while n - p >= self.left:
            p += self.left
            out.append(p)
            self.left = self.fs
            self.ticks += 1
        self.left -= n - p
        return out


class ContTickOracle(TickOracle):
    """A continuous MSK channel of the hooked oracle, opened at `fs`, fed
    messages cut at the model's tick samples.  tick=False: the untimed oracle
    (same cuts, the hook never called)."""

    def __init__(self, bitrate, fs, tick=True, rule='rescale'):
        tl.Oracle.__init__(self, bitrate=bitrate)
        self.tick = tick
        self.clock = TickClock(fs, rule)

    @property
    def ticks(self):
        return self.clock.ticks

    def push(self, pcm, fs=None):
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        if fs is not None:
            self.clock.set_rate(fs)
        p = 0
        for q in self.clock.cuts(len(pcm)):
            tl.Oracle.push(self, pcm[p:q], self.clock.fs)
            if self.tick:
                self.L.oracle_x_dcd_tick(self.h)
            p = q
        if p < len(pcm):
            tl.Oracle.push(self, pcm[p:], self.clock.fs)


class HookedC(TickOracle):
    """The C channel of the hooked library, the hook called at the end of each
    message that completes a second (equals the sample-clock rule when the
    messages divide 48000)."""

    def __init__(self, tick=True):
        tl.Oracle.__init__(self, bitrate=8400, trace_pt=True)
        self.tick = tick
        self.pushed = 0
        self.ticks = 0


def msk_outputs(o):
    return dict(soft=o.softbits(), hops=o.hops(), frames=o.frames(), items=o.item_lines('A'), edges=o.events()[0])


def msk_run(segments, bitrate, fs0, size, tick=True, stop=None, rule='rescale'):
    """segments: [(pcm, fs)], each cut into messages of `size` samples (None:
    one message per segment); stop: total samples fed at most"""
    o = ContTickOracle(bitrate, fs0, tick=tick, rule=rule)
    fed = 0
    for pcm, fs in segments:
        for m in tl.cut(pcm, (size or max(len(pcm), 1),)):
            if stop is not None:
                m = m[:max(0, stop - fed)]
            if len(m):
                o.push(m, fs)
                fed += len(m)
    return msk_outputs(o), o


def c_run(msgs, tick=True, hooked=False):
    o = HookedC(tick=tick) if hooked else tl.Oracle(bitrate=8400, trace_pt=True, dcd_tick=tick)
    for m in msgs:
        o.push(m)
    return tl.c_outputs(o)


def edge_seconds(segments, bitrate, fs0, size, tick=True):
    """(edges, [stream time in seconds of the message end at which each edge shows])"""
    o = ContTickOracle(bitrate, fs0, tick=tick)
    t, seen, at = 0.0, 0, []
    for pcm, fs in segments:
        for m in tl.cut(pcm, (size,)):
            o.push(m, fs)
            t += len(m) / float(fs)
            e = o.events()[0]
            at += [round(t, 3)] * (e - seen)
            seen = e
    return seen, at


def noise_like(pcm, seconds, fs, seed):
    """int16 Gaussian noise, sigma 0.3 of the carrier part's standard deviation"""
    rng = np.random.default_rng(seed)
    return np.round(rng.normal(0, 0.3 * np.std(pcm.astype(np.float64)), int(seconds * fs))).astype(np.int16)


def msk_outage(bitrate, fs, seeds, carrier, on1=12.0, off=7.0, on2=10.0, baud=None, ebn0=14.0):
    """carrier / noise / carrier at one rate: the outage streams of the issue's table"""
    a = tl.synth_msk(seconds=on1, bitrate=bitrate, baud=baud, seed=seeds[0], carrier=carrier, ebn0=ebn0, fs=fs)
    parts = [a, noise_like(a, off, fs, seeds[0])]
    if on2:
        parts.append(tl.synth_msk(seconds=on2, bitrate=bitrate, baud=baud, seed=seeds[1], carrier=carrier, ebn0=ebn0,
                                  fs=fs))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def c_outage(on1=6.0, off=6.0, on2=6.0):
    """6 s of a C channel, 6 s of noise, 6 s of another call: (pcm, samples at the end of the quiet part)"""
    a = tl.synth_c(seconds=on1, seed=0xC1A5, carrier=11000.0, ebn0=12.0)
    b = tl.synth_c(seconds=on2, seed=0xC1A6, carrier=11000.0, ebn0=12.0)
    quiet = noise_like(a, off, C_FS, 0xC1A6)
    return np.concatenate([a, quiet, b]), len(a) + len(quiet)


# The outage streams: 12 s carrier, 7 s noise, 10 s carrier.  `untimed` /
# `ticked`: the DCD edge counts measured with the oracle on the CPU
# (tests/test_oracle_cont_dcd.py asserts them)
MSK_ROWS = {
    'msk600_12000': dict(bitrate=600, fs=12000, seeds=(0xD0, 0xD1), carrier=1800.0, baud=None, untimed=1, ticked=5),
    'msk1200_24000': dict(bitrate=1200, fs=24000, seeds=(0xD4, 0xD5), carrier=1800.0, baud=600, untimed=1, ticked=4),
    'msk600_18750': dict(bitrate=600, fs=18750, seeds=(0xDC, 0xDD), carrier=600.0, baud=None, untimed=1, ticked=4),
    'msk600_16000': dict(bitrate=600, fs=16000, seeds=(0xD8, 0xD9), carrier=600.0, baud=None, untimed=1, ticked=2),
}


@functools.lru_cache(maxsize=None)
def msk_stream(name):
    r = MSK_ROWS[name]
    return msk_outage(r['bitrate'], r['fs'], r['seeds'], r['carrier'], baud=r['baud'])


# Streams that change rate in the middle of a timer second, with an outage:
# [(pcm, fs)] segments; the channel is opened at the first segment's rate
@functools.lru_cache(maxsize=None)
def rate_change_segments(name):
    if name == '12000-16000-12000':
        # (carrier 600 Hz: the demodulator restarts at every rate change and locks within 4 s there)
        a = tl.synth_msk(seconds=7.4, bitrate=600, seed=0xD0, carrier=600.0, ebn0=14.0, fs=12000)
        b = tl.synth_msk(seconds=6.3, bitrate=600, seed=0xD8, carrier=600.0, ebn0=14.0, fs=16000)
        c = tl.synth_msk(seconds=10.0, bitrate=600, seed=0xD1, carrier=600.0, ebn0=14.0, fs=12000)
        return 600, ((a, 12000), (np.concatenate([b, noise_like(b, 6.0, 16000, 0xD8)]), 16000), (c, 12000))
    if name == '24000-40000':
        # the rate changes 0.4 s into a timer second; datacd falls twice at 40 kHz (the flap, the noise)
        a = tl.synth_msk(seconds=9.4, bitrate=1200, baud=600, seed=0xD4, carrier=600.0, ebn0=14.0, fs=24000)
        b = tl.synth_msk(seconds=8.0, bitrate=1200, baud=600, seed=0xD5, carrier=600.0, ebn0=14.0, fs=40000)
        return 1200, ((a, 24000), (np.concatenate([b, noise_like(b, 7.0, 40000, 0xD5)]), 40000))
    raise KeyError(name)


def model_ticks(segments, fs0, rule='rescale'):
    """the ticks a rule gives a stream"""
    clk = TickClock(fs0, rule)
    for pcm, fs in segments:
        clk.set_rate(fs)
        clk.cuts(len(pcm))
    return clk.ticks


def edge_samples(segments, bitrate, fs0, rule='rescale'):
    """[(samples fed when the edge showed, it showed at a tick)] of the ticked
    checker under `rule`, fed tick by tick and in messages of at most Fs / 10"""
    o = ContTickOracle(bitrate, fs0, rule=rule)
    fed, seen, at = 0, 0, []
    for pcm, fs in segments:
        o.clock.set_rate(fs)
        p = 0
        while p < len(pcm):
            n = min(o.clock.left, len(pcm) - p, fs // 10)
            ticks = o.ticks
            o.push(pcm[p:p + n], fs)
            p += n
            fed += n
            e = o.events()[0]
            at += [(fed, o.ticks != ticks)] * (e - seen)
            seen = e
    return at


def rule_witness(segments, bitrate, fs0):
    """The sample count at which the stream tells the rescale rule from a
    restart of the second at a rate change: the first edge the two checkers
    place differently, which must be a fall at a tick of the model.  A copy of
    the stream truncated there (the flush applies the tick on its last sample)
    has different edge counts under the two rules."""
    good, bad = edge_samples(segments, bitrate, fs0), edge_samples(segments, bitrate, fs0, 'restart')
    k = next(i for i, (g, b) in enumerate(zip(good, bad)) if g != b)
    stop, at_tick = good[k]
    assert at_tick and k % 2 == 1 and bad[k][0] > stop, 'not a fall that the model places earlier'
    return stop, k + 1
