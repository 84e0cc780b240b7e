"""Adversarial int16 streams for the burst demodulators (burst.hip,
burst_msk.hip, burst_engine.hip): tests/test_burst_inputs.py proves on the
CPU, with the oracle alone, which bounded resources and framing paths they
reach; tests/test_gpu_burst_inputs.py compares everything the engine delivers
with the oracle's after every run().

All streams are 48 kHz, about 3 s (LEN samples: 144000 and a 37-sample tail);
two are longer, as long as they need: `late` (its burst lies behind 100000
silent samples) and `cut_silence` (silence until the DCD timer's fourth
tick).  Burst output
depends on the message boundaries, so a schedule (SCHEDULES) names the
messages and how many are queued before each run(); the oracle is fed the
same messages.  The gate periods, the cuts and `late`'s length are searched
with the oracle, the way coarse_inputs.edge_stream searches its carriers: a
search that finds nothing raises AssertionError."""
import functools

import numpy as np

import aero_testlib as tl
import oracle_tick as ot

FS = 48000
TAIL = 37
LEN = 3 * FS + TAIL
SEED = 0xB0B5

# kind: AeroL bit rate, carrier (Hz), seed of the plain synthetic stream
KINDS = {'oqpsk10500': (10500, 12000.0, 3), 'msk1200': (1200, 2500.0, 21), 'msk600': (600, 2500.0, 21)}

# burst_common.h (no Python binding): trident checks a channel may have
# recorded and not applied, R/T tests a framing lane queues per pass, the R/T
# block (the last test of a block is at blockptr 320 + 192 * 30 = RT_BLOCK)
TRI_SLOTS = 4
RT_TESTS_PER_PASS = 8
RT_BLOCK = 6080
MAX_MSG = 16384  # the burst path's largest message (B_PCM_CAP / 2)

# unlike neighbours side by side: silence beside the pulse train that stalls
# the front end, full scale beside 1-LSB noise, a decoding lane between them
ORDER = ('silence', 'pulse_stall', 'square', 'lsb_noise', 'const_min', 'synth', 'one_sample', 'tone', 'noise',
         'pulse_reject', 'noise_pulse', 'clip', 'tiny', 'negated', 'lead0', 'late', 'cut_silence', 'cut_fullscale',
         'cut_noise', 'overlap')
SILENT = ('silence', 'square', 'const_min', 'one_sample', 'lsb_noise', 'tone')  # no soft bits

SCHEDULES = ('max', 'queued', 'ragged')
RAGGED = (6144, 6145, 6146, 1, 12000, 2047, 16384, 37)  # around the Hilbert block (6145) and the small sizes


def runs(n, schedule):
    """The [start, stop) of every message of an n-sample stream, grouped by
    the run() they are queued before.  max: one 16384-sample message per run;
    queued: two of 16383 (the most the PCM ring admits without an early
    pass); ragged: RAGGED cycled, one per run."""
    out, p, k = [], 0, 0
    while p < n:
        grp = []
        for size in {'max': (MAX_MSG,), 'queued': (MAX_MSG - 1, MAX_MSG - 1),
                     'ragged': (RAGGED[k % len(RAGGED)],)}[schedule]:
            if p < n:
                grp.append((p, min(n, p + size)))
                p = grp[-1][1]
        out.append(grp)
        k += 1
    return out


def oracle(kind, tick=False):
    return ot.TickOracle(bitrate=KINDS[kind][0], tick=tick)


def walk(kind, pcm, schedule='max', tick=False):
    """The oracle over pcm in the schedule's messages: (final outputs as
    ot.outputs gives them, per message (trident checks, R/T tests))."""
    o = oracle(kind, tick)
    per, nh, nt = [], 0, 0
    for grp in runs(len(pcm), schedule):
        for a, b in grp:
            o.push(pcm[a:b])
            h, t = len(o.hops()), len(o.rt_tests())
            per.append((h - nh, t - nt))
            nh, nt = h, t
    return ot.outputs(o), per


def facts(kind, pcm, schedule='max', tick=False):
    """What a stream reaches in the oracle, as plain numbers."""
    out, per = walk(kind, pcm, schedule, tick)
    h, t, s = out['hops'], out['tests'], out['soft']
    return dict(checks=len(h), accepted=int((h[:, 1] != 0).sum()) if len(h) else 0,
                checks_msg=max(p[0] for p in per), tests=len(t), tests_msg=max(p[1] for p in per),
                blockptr=int(t[:, 0].max()) if len(t) else 0, soft=int((s != -1).sum()), marks=int((s == -1).sum()),
                packets=len(out['packets']), edges=out['edges'], finite=bool(np.isfinite(h).all()))


@functools.lru_cache(maxsize=None)
def _synth(kind, n=LEN, lead_in=24000):
    """the plain synthetic stream of the kind (read-only: cached)"""
    bitrate, carrier, seed = KINDS[kind]
    sec = n / FS + 0.001
    if bitrate == 10500:
        x = tl.synth_burst(seconds=sec, seed=seed, carrier=carrier, ebn0=14.0, lead_in=lead_in)
    else:
        x = tl.synth_burst_msk(seconds=sec, bitrate=bitrate, seed=seed, carrier=carrier, ebn0=14.0, lead_in=lead_in)
    assert len(x) >= n
    x = x[:n]
    x.setflags(write=False)
    return x


def _gate(x, period):
    """x on for `period` samples, off for the next `period`, ..."""
    return np.where((np.arange(len(x)) // period) % 2 == 0, x, 0).astype(np.int16)


def _tone(kind, n=LEN, amplitude=8000):
    return np.round(amplitude * np.cos(2 * np.pi * KINDS[kind][1] / FS * np.arange(n))).astype(np.int16)


def _noise(kind, n=LEN, salt=0):
    rng = np.random.default_rng([SEED, KINDS[kind][0], salt])
    return np.clip(np.round(rng.normal(0, 0.25 * 32768 / 3, n)), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def stall_stream(kind):
    """(stream, gate period).  OQPSK: the carrier gated on and off every
    1400 .. 1600 samples, the first period at which the oracle, fed 16384-sample
    messages, records more than TRI_SLOTS checks in one message, runs more
    than RT_TESTS_PER_PASS R/T tests in one message, fills an R/T block to
    its last test (blockptr RT_BLOCK), and accepts checks both with and
    without a start-of-packet marker behind them (fewer markers than accepted
    checks).  MSK: the period of 5000 .. 6000 with the most checks in one
    message, then the most checks (its checks lie at least 9866 samples
    apart: no stall there, all rejected)."""
    tone = _tone(kind)
    if KINDS[kind][0] == 10500:
        for period in range(1400, 1601, 25):
            x = _gate(tone, period)
            f = facts(kind, x)
            if f['checks_msg'] > TRI_SLOTS and f['tests_msg'] > RT_TESTS_PER_PASS and f['blockptr'] == RT_BLOCK and \
                    0 < f['marks'] < f['accepted']:
                return x, period
        raise AssertionError('%s: no gate period stalls the front end and the framing' % kind)
    best = None
    for period in range(5000, 6001, 100):
        x = _gate(tone, period)
        f = facts(kind, x)
        key = (f['checks_msg'], f['checks'])
        if best is None or key > best[0]:
            best = (key, x, period)
    if best[0][1] == 0:
        raise AssertionError('%s: no gate period gives a trident check' % kind)
    return best[1], best[2]


# gate periods of pulse_reject (searched) and noise_pulse; how far before
# the first accepted check the cut search starts (more than the delays d1 and
# d2 and the trident buffer together: 8003 and 27262 samples) and its step
REJECT_PERIODS = {10500: range(2400, 3001, 100), 1200: range(8000, 12001, 1000), 600: range(8000, 12001, 1000)}
NOISE_PERIOD = {10500: 1500, 1200: 8000, 600: 8000}
CUT_SEARCH = {10500: (16000, 250), 1200: (32000, 1000), 600: (32000, 1000)}


@functools.lru_cache(maxsize=None)
def reject_stream(kind):
    """(stream, gate period): a gated carrier with the most checks among the
    REJECT_PERIODS whose checks the oracle all rejects."""
    tone, best = _tone(kind), None
    for period in REJECT_PERIODS[KINDS[kind][0]]:
        x = _gate(tone, period)
        f = facts(kind, x)
        if f['checks'] and not f['accepted'] and (best is None or f['checks'] > best[0]):
            best = (f['checks'], x, period)
    if best is None:
        raise AssertionError('%s: no gate period has all its checks rejected' % kind)
    return best[1], best[2]


@functools.lru_cache(maxsize=None)
def first_accept(kind):
    """sample of the first accepted trident check of the plain synthetic stream"""
    h = walk(kind, _synth(kind))[0]['hops']
    acc = h[h[:, 1] != 0]
    assert len(acc), '%s: the synthetic stream has no accepted check' % kind
    return int(acc[0, 0])


def _cut(kind, fill, cut, n=LEN):
    y = np.zeros(n, dtype=np.int16)
    if fill == 'fullscale':
        y[:] = 32767
    elif fill == 'noise':
        y[:] = _noise(kind, n, salt=1)
    y[:cut] = _synth(kind)[:cut]
    return y


@functools.lru_cache(maxsize=None)
def cut_stream(kind, fill):
    """(stream, cut): the synthetic stream cut off inside a packet and
    continued with zeros ('silence'), +32767 ('fullscale') or noise.  The cut
    is searched forwards (CUT_SEARCH: from where, in which steps) towards the
    first accepted check, which lags its burst; the other fills start at the
    cut found for silence.  It is the earliest cut at which the oracle finds
    the UW (a DataCarrierDetect change), runs at least one R/T test and
    decodes fewer packets than from the uncut stream: the packet's body is
    the fill.

    cut_silence is also the class that tells AeroL's 1-s DCD timer: nothing
    follows the UW, so only the timer's fourth tick drops DataCarrierDetect.
    Its silence is as many whole seconds long as that takes (the first length
    at which the ticked oracle's DataCarrierDetect changes differ from the
    untimed one's)."""
    whole = facts(kind, _synth(kind))['packets']
    assert whole >= 1, '%s: the synthetic stream has no packet' % kind
    acc = first_accept(kind)
    back, step = CUT_SEARCH[KINDS[kind][0]]
    lo = max(acc - back, 0) if fill == 'silence' else cut_stream(kind, 'silence')[1]
    for cut in range(lo, acc + back, step):
        y = _cut(kind, fill, cut)
        f = facts(kind, y)
        if f['edges'] >= 1 and f['tests'] >= 1 and f['packets'] < whole:
            break
    else:
        raise AssertionError('%s: no cut leaves the UW and an R/T test without the packet (%s)' % (kind, fill))
    if fill != 'silence':
        return y, cut
    for seconds in range(3, 9):
        y = _cut(kind, fill, cut, seconds * FS + TAIL)
        if facts(kind, y, tick=True)['edges'] != facts(kind, y)['edges']:
            return y, cut
    raise AssertionError('%s: the DCD timer changes nothing within 8 s of the cut' % kind)


LATE_LEAD = 100000  # silent samples before the burst: the 48000-slot AGC ring has turned over twice


@functools.lru_cache(maxsize=None)
def late_stream(kind):
    """The synthetic stream with a lead-in of LATE_LEAD samples, all zero: the
    AGC ring holds zeros only and the gain stands on its floor
    (fmax(agc_sum / 48000, 1e-6)) when the burst arrives.  Its length is the
    shortest, in steps of 16384 samples and at most 3 s behind the lead-in,
    from which the oracle decodes a packet; where it decodes none (MSK: the
    burst's check is rejected), the shortest that holds every trident check
    of the longest."""
    steps = range(LATE_LEAD + MAX_MSG, LATE_LEAD + 3 * FS + 1, MAX_MSG)
    x = _synth(kind, steps[-1] + TAIL, lead_in=LATE_LEAD).copy()
    x[:LATE_LEAD] = 0
    got = [facts(kind, x[:n + TAIL]) for n in steps]
    for n, f in zip(steps, got):
        if f['packets'] >= 1 or (not got[-1]['packets'] and f['checks'] == got[-1]['checks']):
            return x[:n + TAIL].copy()
    raise AssertionError('%s: no length holds the checks of the longest' % kind)


@functools.lru_cache(maxsize=None)
def streams(kind):
    """[(class, int16 stream)] in ORDER; the arrays are read-only."""
    bitrate = KINDS[kind][0]
    rng = np.random.default_rng([SEED, bitrate])
    n, t = LEN, np.arange(LEN)
    syn = _synth(kind).copy()
    wide = syn.astype(np.int32)
    out = {}
    out['silence'] = np.zeros(n, dtype=np.int16)
    out['square'] = np.where((t // 3) % 2 == 0, 32767, -32768).astype(np.int16)
    out['const_min'] = np.full(n, -32768, dtype=np.int16)
    one = np.zeros(n, dtype=np.int16)
    one[FS // 2 + 29] = 29
    out['one_sample'] = one
    out['lsb_noise'] = rng.integers(-1, 2, n).astype(np.int16)
    out['tone'] = _tone(kind)
    out['noise'] = _noise(kind)
    out['pulse_stall'] = stall_stream(kind)[0]
    out['pulse_reject'] = reject_stream(kind)[0]
    out['noise_pulse'] = _gate(_noise(kind, salt=2), NOISE_PERIOD[bitrate])
    out['synth'] = syn
    out['clip'] = np.clip(wide * 8, -32768, 32767).astype(np.int16)
    out['tiny'] = (wide // 2048).astype(np.int16)
    out['negated'] = np.clip(-wide, -32768, 32767).astype(np.int16)  # 32768 has no int16: clipped
    out['lead0'] = _synth(kind, lead_in=0).copy()
    out['late'] = late_stream(kind)
    for fill in ('silence', 'fullscale', 'noise'):
        out['cut_' + fill] = cut_stream(kind, fill)[0]
    out['overlap'] = np.clip(wide + np.roll(wide, 7000), -32768, 32767).astype(np.int16)
    assert set(out) == set(ORDER)
    for v in out.values():
        assert v.dtype == np.int16
        v.setflags(write=False)
    return [(name, out[name]) for name in ORDER]
