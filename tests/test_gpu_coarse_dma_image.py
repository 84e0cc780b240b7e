"""The overlapped head's ring image filled by direct-to-LDS loads, and the
successor's table gathers issued under |X| (coarse.hip, coarse_lds.h).

The image no longer passes through registers: every wave loads its share of
the successor's ring straight into the LDS, one thread patches the ring
fix-up's word into the image behind its wave's loads, one barrier in the
middle of |X| makes the image whole, and the gathers go out from there as the
|X| registers die.  Nothing may change by a bit: hop records, the final
smoothed spectrum y, soft bits and items equal the CPU oracle's with one and
two workgroups, with the overlap on and off, for the OQPSK and the C-channel
instance, where

  fixup    every channel of the batch takes the ring fix-up in the same run
           (pushes of 4095 then 4097 samples), so the patched word and the
           image loads meet on every successor;
  silence  an all-zero channel lies between two live ones and a live one
           between two silent ones, so the general hypot path runs beside the
           branch-free one on either side of the barrier inside |X|;
  retune   a channel at 7020 Hz retunes, so zero_before and yreset fall on a
           successor."""
import concurrent.futures as cf

import numpy as np
import pytest

import aero_testlib as tl

pytestmark = pytest.mark.gpu

SECONDS = 3.0
NSAMP = int(SECONDS * 48000)
HOP = 4096
# per case: (carrier or None for silence, Eb/N0) per channel, and the push sizes of alternate rounds
CASES = {
    'fixup': ([(12037.5, 12.0), (12020.0, 11.0), (12055.0, 10.0), (11990.0, 12.0)], (4095, 4097)),
    'silence': ([(12037.5, 12.0), None, (12050.0, 11.0), None], (12000, 12000)),
    'retune': ([(12037.5, 12.0), (7020.0, 12.0), (12040.0, 10.0)], (12000, 12000)),
}


def _oracle(pcm, bitrate, sizes):
    """The reference fed the messages the engine is fed: the C channel's
    prefilter works per message, so unlike the P channel it is not
    chunk-invariant bit for bit (tests/test_oracle_c.py)."""
    o = tl.Oracle(bitrate=bitrate)
    pos, r = 0, 0
    while pos < len(pcm):
        o.push(pcm[pos:pos + sizes[r % 2]])
        pos += sizes[r % 2]
        r += 1
    return o.softbits(), o.hops(), (o.c_units() if bitrate == 8400 else o.item_lines('A')), o.coarse_y()


def _streams(bitrate):
    """Per case the channels' PCM and the oracle's results; a stream that two
    cases share with the same pushes (the first channel, silence) is made
    and decoded once."""
    made = {}

    def pcm(spec, k):
        if spec is None:
            return np.zeros(NSAMP, dtype=np.int16)
        f, eb = spec
        if bitrate == 8400:
            return tl.synth_c(seconds=SECONDS, seed=0xD3A0 + k, carrier=f, ebn0=eb)
        return tl.synth(seconds=SECONDS, seed=0xD3A0 + k, carrier=f, ebn0=eb)

    keys = []
    for name, (chans, sizes) in CASES.items():
        for k, spec in enumerate(chans):
            key = (spec, k if spec is not None else -1, sizes)
            keys.append((name, key))
            if key not in made:
                made[key] = pcm(spec, k)
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        refs = dict(zip(made, ex.map(lambda kv: _oracle(kv[1], bitrate, kv[0][2]), made.items())))
    out = {}
    for name, key in keys:
        out.setdefault(name, ([], []))
        out[name][0].append(made[key])
        out[name][1].append(refs[key])
    return out


@pytest.fixture(scope='module')
def oqpsk(cpu_libs):
    return _streams(10500)


@pytest.fixture(scope='module')
def c8400(cpu_libs):
    return _streams(8400)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _run(ae, streams, sizes, bitrate):
    eng = ae.Engine(max_channels=len(streams), flags=ae.F_TRACE_SOFT | ae.F_TRACE_HOPS)
    chans = [eng.open_channel(bitrate, 48000) for _ in streams]
    pos, r = 0, 0
    while pos < NSAMP:
        n = sizes[r % 2]
        for s, ch in zip(streams, chans):
            eng.push(ch, s[pos:pos + n])
        eng.run()
        pos += n
        r += 1
    eng.flush()
    return eng, chans


def _check(eng, chans, refs, what, units):
    for k, (ch, (rsb, rh, rit, ry)) in enumerate(zip(chans, refs)):
        assert len(rh) >= NSAMP // HOP - 1
        assert _same(eng.hops(ch), rh), '%s: channel %d hop records differ' % (what, k)
        first, y = eng.channel_coarse_y(ch)
        assert _same(y, ry[first:first + len(y)]), '%s: channel %d final y differs' % (what, k)
        assert np.array_equal(eng.softbits(ch), rsb), '%s: channel %d soft bits differ' % (what, k)
        if units:
            assert np.array_equal(eng.c_units(ch), rit), '%s: channel %d Call_progress SUs differ' % (what, k)
        else:
            assert eng.items(ch) == rit, '%s: channel %d items differ' % (what, k)


def _case(ae, data, name, bitrate, monkeypatch, grid, overlap):
    streams, refs = data[name]
    if name == 'retune':  # the retune happened: the centre frequency moved
        assert len(np.unique(refs[1][1][:, 3])) > 1, 'the 7020 Hz channel never retuned'
    if name == 'silence':
        assert len(refs[0][0]) > 1000, 'oracle did not lock on the live channel'
    monkeypatch.setenv('AERO_COARSE_GRID', str(grid))
    monkeypatch.setenv('AERO_COARSE_OVERLAP', str(overlap))
    eng, chans = _run(ae, streams, CASES[name][1], bitrate)
    _check(eng, chans, refs, '%s %d bps grid %d overlap %d' % (name, bitrate, grid, overlap), bitrate == 8400)
    eng.close()


@pytest.mark.parametrize('overlap', [1, 0])
@pytest.mark.parametrize('grid', [1, 2])
@pytest.mark.parametrize('name', list(CASES))
def test_oqpsk(engine_lib, oqpsk, monkeypatch, name, grid, overlap):
    import aero_engine as ae
    _case(ae, oqpsk, name, 10500, monkeypatch, grid, overlap)


@pytest.mark.parametrize('overlap', [1, 0])
@pytest.mark.parametrize('grid', [1, 2])
@pytest.mark.parametrize('name', list(CASES))
def test_c8400(engine_lib, c8400, monkeypatch, name, grid, overlap):
    import aero_engine as ae
    _case(ae, c8400, name, 8400, monkeypatch, grid, overlap)
