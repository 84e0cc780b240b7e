"""AeroL's 1 s DCD timer on continuous MSK channels and the C channel
(AERO_F_DCD_TICK_CONT) on the GPU, against the model of tests/cont_dcd_lib.py:
the hooked oracle fed the stream cut at the tick samples (MSK), the oracle's
own sample-clock timer (C).  Every comparison is bitwise on soft bits, hop
records, frames and items (C: pt, Call_progress SUs, voice) and on the
DataCarrierDetect edge count, and first asserts that the checker's ticked
edge count differs from its untimed one, so no test passes with the flag
ignored.  A stream is decoded at several lengths (truncated copies on
channels of one engine), which pins when the edges happen, not only how many
there are."""
import functools
import signal
import subprocess
import time

import numpy as np
import pytest

import aero_testlib as tl
import cont_dcd_lib as cd

pytestmark = pytest.mark.gpu


def _flags(ae, tick=True):
    return ae.F_TRACE_SOFT | ae.F_TRACE_HOPS | ae.F_TRACE_FRAMES | (ae.F_DCD_TICK_CONT if tick else 0)


def _msk_take(eng, ch):
    return dict(soft=eng.softbits(ch), hops=eng.hops(ch), frames=eng.frames(ch), items=eng.items(ch))


def _msk_equal(got, edges, ref, what):
    assert len(ref['soft']) > 1000, '%s: the checker did not lock' % what
    assert len(got['soft']) == len(ref['soft']) and np.array_equal(got['soft'], ref['soft']), '%s: soft bits' % what
    h, rh = got['hops'], ref['hops']
    assert h.shape == rh.shape and np.array_equal(h.view(np.int64), rh.view(np.int64)), '%s: hop records' % what
    assert np.array_equal(got['frames'], ref['frames']), '%s: frames' % what
    assert got['items'] == ref['items'], '%s: items' % what
    assert edges == ref['edges'], '%s: DCD changes %d, the checker %d' % (what, edges, ref['edges'])


@functools.lru_cache(maxsize=None)
def _stops(name):
    """sample counts at the first fall of datacd (a tick on the last sample:
    the flush applies it), at the end of the Fs / 10 message that holds the
    re-rise, and the whole stream (from the checker)"""
    r = cd.MSK_ROWS[name]
    pcm, fs = cd.msk_stream(name), r['fs']
    n, at = cd.edge_seconds([(pcm, fs)], r['bitrate'], fs, fs // 10)
    assert n == r['ticked'] >= 2
    stops = [int(round(at[1] * fs))]
    assert stops[0] % fs == 0, 'datacd falls at a tick'
    if n >= 3:
        stops.append(int(round(at[2] * fs)))
    return tuple(stops + [len(pcm)])


@functools.lru_cache(maxsize=None)
def _msk_ref(name, stop, tick=True):
    r = cd.MSK_ROWS[name]
    return cd.msk_run([(cd.msk_stream(name)[:stop], r['fs'])], r['bitrate'], r['fs'], None, tick=tick)[0]


def _feed(eng, chans, msgs, run_every=1):
    """msgs: per channel a list of (pcm, fs) messages"""
    for k in range(max(len(m) for m in msgs)):
        for ch, m in zip(chans, msgs):
            if k < len(m):
                eng.push(ch, m[k][0], fs=m[k][1])
        if (k + 1) % run_every == 0:
            eng.run()
    eng.flush()


def _msk_outage(name, size, run_every):
    import aero_engine as ae
    r = cd.MSK_ROWS[name]
    pcm, fs, stops = cd.msk_stream(name), r['fs'], _stops(name)
    refs = [_msk_ref(name, s) for s in stops]
    plain = _msk_ref(name, stops[-1], tick=False)
    assert plain['edges'] == r['untimed'] == 1 and refs[-1]['edges'] == r['ticked'] != plain['edges']
    assert [x['edges'] for x in refs[:-1]] == [2, 3][:len(stops) - 1], 'the lengths do not separate the edges'
    eng = ae.Engine(max_channels=len(stops), flags=_flags(ae))
    chans = [eng.open_channel(r['bitrate'], fs=fs) for _ in stops]
    _feed(eng, chans, [[(m, fs) for m in tl.cut(pcm[:s], (size,))] for s in stops], run_every)
    for ch, s, ref in zip(chans, stops, refs):
        _msk_equal(_msk_take(eng, ch), eng.channel_events(ch)[0], ref, '%s, %d samples' % (name, s))
    eng.close()


@pytest.mark.parametrize('run_every', [1, 3])
@pytest.mark.parametrize('size', ['1200', 'ragged', 'second'])
@pytest.mark.parametrize('name', ['msk600_12000', 'msk1200_24000'])
def test_msk_outage(engine_lib, cpu_libs, msk_kernel, name, size, run_every):
    fs = cd.MSK_ROWS[name]['fs']
    _msk_outage(name, {'1200': 1200, 'ragged': 1777, 'second': fs}[size], run_every)


@pytest.mark.parametrize('name', ['msk600_18750', 'msk600_16000'])
def test_msk_generic_rates(engine_lib, cpu_libs, name):
    _msk_outage(name, 2500, 1)


@pytest.mark.parametrize('name', ['12000-16000-12000', '24000-40000'])
def test_msk_rate_change_mid_second(engine_lib, cpu_libs, name):
    """The whole stream, and a copy that ends on the model's tick sample of a
    fall after the rate change, where the flush applies that tick: a timer
    whose second restarted at the rate change (or whose rescale were off by a
    sample) has not fallen there, so its edge count differs."""
    import aero_engine as ae
    bitrate, segs = cd.rate_change_segments(name)
    fs0 = segs[0][1]
    stop, edges_at_stop = cd.rule_witness(segs, bitrate, fs0)
    assert stop > len(segs[0][0]), 'the witness lies after the rate change'
    ref, _ = cd.msk_run(segs, bitrate, fs0, None)
    plain, _ = cd.msk_run(segs, bitrate, fs0, None, tick=False)
    cut, _ = cd.msk_run(segs, bitrate, fs0, None, stop=stop)
    wrong, _ = cd.msk_run(segs, bitrate, fs0, None, stop=stop, rule='restart')
    early, _ = cd.msk_run(segs, bitrate, fs0, None, stop=stop - 1)
    assert ref['edges'] != plain['edges'] == 1
    assert cut['edges'] == edges_at_stop == wrong['edges'] + 1 == early['edges'] + 1, \
        'the truncated copy does not tell the rules apart'
    eng = ae.Engine(max_channels=3, flags=_flags(ae))
    stops, refs = (sum(len(p) for p, _ in segs), stop, stop - 1), (ref, cut, early)
    chans = [eng.open_channel(bitrate, fs=fs0) for _ in stops]
    msgs = []
    for s in stops:
        m, fed = [], 0
        for pcm, fs in segs:
            m += [(x, fs) for x in tl.cut(pcm[:max(0, s - fed)], (fs // 4 + 7,))]
            fed += len(pcm)
        msgs.append(m)
    _feed(eng, chans, msgs)
    for ch, s, r in zip(chans, stops, refs):
        _msk_equal(_msk_take(eng, ch), eng.channel_events(ch)[0], r, '%s, %d samples' % (name, s))
    eng.close()


# ---------------------------------------------------------------- C channel
@functools.lru_cache(maxsize=None)
def _c_ref(size, stop, tick=True):
    pcm, _ = cd.c_outage()
    return cd.c_run(tl.cut(pcm[:stop], (size,)), tick=tick)


@pytest.mark.parametrize('order', ['traced', 'deferred'])
@pytest.mark.parametrize('size', [4800, 7000])
def test_c_call_end(engine_lib, cpu_libs, size, order):
    """`order`: with the parity traces a pass's Viterbi runs at once, without
    them inside the next pass (the production order)"""
    import aero_engine as ae
    pcm, quiet_end = cd.c_outage()
    stops = (quiet_end, len(pcm))
    refs = [_c_ref(size, s) for s in stops]
    plain = _c_ref(size, len(pcm), tick=False)
    assert plain['edges'] == 1 and refs[1]['edges'] == 3
    assert refs[0]['edges'] == 2, 'the call has ended: an even edge count after the quiet part'
    # a tick falls while the demod delivers no soft bit: none in the second around sample 10 x 48000
    o = tl.Oracle(bitrate=8400, dcd_tick=True)
    count = []
    for m in tl.cut(pcm[:11 * cd.C_FS], (4800,)):
        o.push(m)
        count.append(len(o.softbits()))
    assert count[10 * 10 - 6] == count[10 * 10 + 4] > 10000
    traces = ('soft', 'pt', 'hops') if order == 'traced' else ()
    flags = ae.F_TRACE_FRAMES | ae.F_DCD_TICK_CONT
    if traces:
        flags |= ae.F_TRACE_PT | ae.F_TRACE_SOFT | ae.F_TRACE_HOPS
    eng = ae.Engine(max_channels=2, flags=flags)
    chans = [eng.open_channel(8400, 48000) for _ in stops]
    _feed(eng, chans, [[(m, 48000) for m in tl.cut(pcm[:s], (size,))] for s in stops])
    for ch, s, ref in zip(chans, stops, refs):
        got = tl.c_take(eng, ch)
        assert got['edges'] == ref['edges'], '%d samples: DCD changes %d, the checker %d' % (s, got['edges'],
                                                                                             ref['edges'])
        tl.c_equal(got, ref, '%d samples' % s, traces=traces)
    assert eng.channel_events(chans[0])[0] % 2 == 0, 'the host cannot see the call end'
    eng.close()


# ---------------------------------------------------------------- lifecycle
def _join(a, b):
    return {k: (a[k] + b[k]) if isinstance(a[k], list) else np.concatenate([a[k], b[k]]) for k in a}


def test_export_between_fall_and_rise(engine_lib, cpu_libs):
    import aero_engine as ae
    name = 'msk600_12000'
    pcm, fs, stops = cd.msk_stream(name), 12000, _stops(name)
    ref = _msk_ref(name, stops[-1])
    assert _msk_ref(name, stops[0])['edges'] == 2 and ref['edges'] == 5
    assert _msk_ref(name, stops[-1], tick=False)['edges'] == 1, 'untimed, the stream shows one edge'
    msgs = tl.cut(pcm, (1500,))
    k = stops[0] // 1500
    A = ae.Engine(max_channels=2, flags=_flags(ae))
    B = ae.Engine(max_channels=200, flags=_flags(ae))  # another column pitch, another slot
    ch = A.open_channel(600)
    assert B.open_channel(600) == 0
    for m in msgs[:k]:
        A.push(ch, m)
        A.run()
    A.push(ch, msgs[k])  # pushed and not yet demodulated
    blob = A.export_channel(ch)
    head = _msk_take(A, ch)
    A.close_channel(ch)
    ch2 = B.import_channel(blob)
    assert ch2 == 1
    assert B.channel_events(ch2)[0] == 2, 'datacd has fallen and not risen again at the export'
    for m in msgs[k + 1:]:
        B.push(ch2, m)
        B.run()
    B.flush()
    _msk_equal(_join(head, _msk_take(B, ch2)), B.channel_events(ch2)[0], ref, 'the moved channel')
    # an engine without the flag refuses the blob
    E = ae.Engine(max_channels=2, flags=_flags(ae, tick=False))
    with pytest.raises(ae.AeroError) as err:
        E.import_channel(blob)
    assert err.value.rc == ae.AERO_E_INVALID
    for e in (A, B, E):
        e.close()


def test_reopened_slot_starts_a_fresh_timer(engine_lib, cpu_libs):
    import aero_engine as ae
    name = 'msk600_12000'
    pcm, fs, stops = cd.msk_stream(name), 12000, _stops(name)
    assert _msk_ref(name, stops[-1])['edges'] == 5 != _msk_ref(name, stops[-1], tick=False)['edges'] == 1
    eng = ae.Engine(max_channels=1, flags=_flags(ae))
    ch = eng.open_channel(600)
    # closed 11.3 s into the stream: datacd set, 0.3 s into a timer second
    for m in tl.cut(pcm[:11 * fs + 3600], (1500,)):
        eng.push(ch, m)
        eng.run()
    assert eng.channel_events(ch)[0] == 1
    eng.close_channel(ch)
    ch = eng.open_channel(600)
    assert ch == 0
    _feed(eng, [ch], [[(m, fs) for m in tl.cut(pcm, (1500,))]])
    _msk_equal(_msk_take(eng, ch), eng.channel_events(ch)[0], _msk_ref(name, stops[-1]), 'the reopened slot')
    eng.close()


def test_shape_switch_keeps_ticks(engine_lib, cpu_libs, monkeypatch):
    """the group changes from the few-channel to the one-lane kernels when a
    third channel opens mid-stream (as tests/test_gpu_shape_switch.py)"""
    import aero_engine as ae
    monkeypatch.setenv('AERO_MSK_WIDE', '2')
    name = 'msk600_12000'
    pcm, fs, stops = cd.msk_stream(name), 12000, _stops(name)
    refs = [_msk_ref(name, s) for s in (stops[-1], stops[0], stops[1])]
    assert [r['edges'] for r in refs] == [5, 2, 3]
    assert _msk_ref(name, stops[-1], tick=False)['edges'] == 1, 'untimed, the stream shows one edge'
    eng = ae.Engine(max_channels=4, flags=_flags(ae))
    lens = (stops[-1], stops[0], stops[1])
    msgs = [tl.cut(pcm[:n], (3000,)) for n in lens]
    opens, chans = (0, 0, 9), [None] * 3  # the third opens 2.25 s into the others' streams
    for k in range(len(msgs[0]) + opens[2]):
        for i in range(3):
            if chans[i] is None and k >= opens[i]:
                chans[i] = eng.open_channel(600)
            j = k - opens[i]
            if chans[i] is not None and 0 <= j < len(msgs[i]):
                eng.push(chans[i], msgs[i][j])
        eng.run()
    eng.flush()
    for ch, n, ref in zip(chans, lens, refs):
        _msk_equal(_msk_take(eng, ch), eng.channel_events(ch)[0], ref, '%d samples' % n)
    eng.close()


def test_oqpsk_flag_alone_leaves_msk_and_c(engine_lib, cpu_libs):
    """AERO_F_DCD_TICK is continuous OQPSK's: MSK and C channels stay untimed (1 edge)"""
    import aero_engine as ae
    name = 'msk600_12000'
    pcm, stops = cd.msk_stream(name), _stops(name)
    cpcm, _ = cd.c_outage()
    ref, cref = _msk_ref(name, stops[-1], tick=False), _c_ref(4800, len(cpcm), tick=False)
    assert ref['edges'] == 1 != _msk_ref(name, stops[-1])['edges'] and cref['edges'] == 1 != _c_ref(4800, len(cpcm))['edges']
    eng = ae.Engine(max_channels=2, flags=_flags(ae, tick=False) | ae.F_DCD_TICK)
    ch, cc = eng.open_channel(600), eng.open_channel(8400, 48000)
    _feed(eng, [ch, cc], [[(m, 12000) for m in tl.cut(pcm, (1200,))], [(m, 48000) for m in tl.cut(cpcm, (4800,))]])
    _msk_equal(_msk_take(eng, ch), eng.channel_events(ch)[0], ref, 'MSK under AERO_F_DCD_TICK')
    tl.c_equal(tl.c_take(eng, cc), cref, 'C under AERO_F_DCD_TICK', traces=('soft', 'hops'))
    eng.close()


def test_aero_decode_reports_carrier_loss(engine_lib, cpu_libs, tmp_path):
    """bin/aero-decode -v with AERO_DCD_TICK=2: its "Data carrier lost" and
    "detected" lines are the checker's falls and rises"""
    import build
    import test_gpu_host as gh
    build.build_host()
    name = 'msk600_12000'
    pcm = cd.msk_stream(name)
    ref, _ = cd.msk_run([(pcm, 12000)], 600, 12000, 6000)
    assert ref['edges'] == 5 != _msk_ref(name, len(pcm), tick=False)['edges']
    f = tmp_path / 'vfo.pcm'
    pcm.astype('<i2').tofile(str(f))
    port = gh.free_port()
    dec, lines, th = gh._start_decoder(['-p', 'tcp://127.0.0.1:%d' % port, '-t', 'VFO05', '-b', '600', '--format',
                                        'jsondump', '-s', gh.STATION, '-v'], {'AERO_DCD_TICK': '2'})
    try:
        r = subprocess.run([gh.PUB, '--bind', 'tcp://127.0.0.1:%d' % port, '--topic', 'VFO05', '--rate', '12000',
                            '--chunk', '6000', '--wait-ms', '1500', str(f)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        t0 = time.time()
        while sum('Data carrier' in l for l in lines) < ref['edges'] and time.time() - t0 < 60:
            time.sleep(0.2)
    finally:
        dec.send_signal(signal.SIGTERM)
        rc = dec.wait(timeout=120)
    th.join(timeout=10)
    assert rc == 0, '\n'.join(lines[-20:])
    assert sum('Data carrier detected: no signal => signal' in l for l in lines) == (ref['edges'] + 1) // 2
    assert sum('Data carrier lost: signal => no signal' in l for l in lines) == ref['edges'] // 2
    assert [l for l in lines if l.startswith('{')] == gh.expected(ref['items'], 3)
