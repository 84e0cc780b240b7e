"""The channeliser's wideband carrier survey (aero-cli_amd/csrc/survey.hip,
aero_chan_survey_* in include/aero_chan.h) against its numpy restatement
(tests/survey_model.py: float32 -> float64, window, the oracle's JFFT per
segment, re*re + im*im, sequential sums, the tail carried across reads).
Every comparison is of bit patterns; no tolerance.  288 ksps, reads of 57600
samples: 14.06, 7.03 and 3.52 segments per read, so every read leaves a tail,
and a batch of three reads crosses read boundaries inside one launch."""
import numpy as np
import pytest

import aero_testlib as tl
import survey_model as sm

pytestmark = pytest.mark.gpu

C = tl.CENTER
CFG = tl.PUB_CONFIGS['r288k']
FS = CFG['sample_rate']
B = sm.B288


def chan(max_blocks=1, host_out=False, dcc=False, cfg=CFG):
    import aero_engine as ae
    ch = ae.Channeliser(cfg['sample_rate'], C, cfg['mains'], cfg['vfos'], correct_dc_bias=dcc, max_blocks=max_blocks,
                        host_out=host_out)
    return ch


def reads(x, block=B):
    return [x[b * block:(b + 1) * block] for b in range(len(x) // block)]


def equal(got, want, what=''):
    acc, seg = got
    assert seg == want[1], '%s: %d segments, the model has %d' % (what, seg, want[1])
    bad = np.flatnonzero(acc.view(np.uint64) != want[0].view(np.uint64))
    assert bad.size == 0, '%s: %d of %d bins differ, first %d: %r != %r' % (what, bad.size, acc.size, bad[0],
                                                                              acc[bad[0]], want[0][bad[0]])


def one_read_per_run(ch, x, block=B):
    for r in reads(x, block):
        ch.push(r)
        ch.run()


@pytest.mark.parametrize('log2n', [12, 13, 14])
def test_one_read_per_run(engine_lib, log2n):
    x = sm.stream('tones')
    with chan() as ch:
        assert ch.stat('survey_launches') == 0 and ch.stat('survey_segments') == 0
        before = ch.stat('device_bytes')
        ch.survey_start(log2n)
        n = 1 << log2n
        assert ch.stat('device_bytes') >= before + 8 * n * (3 + (n - 1 + B) // n)  # sums, tail, tables, scratch
        one_read_per_run(ch, x)
        want = sm.reference('tones', log2n)
        equal(ch.survey_read(), want, 'log2n %d' % log2n)
        assert ch.stat('survey_segments') == want[1] == 7 * B >> log2n
        assert ch.stat('survey_launches') == 2 * 7
        ch.survey_stop()
        assert ch.stat('device_bytes') == before


@pytest.mark.parametrize('log2n', [12, 13, 14])
def test_batches_of_three_reads(engine_lib, log2n):
    """max_blocks 3, all 7 reads pushed before one run: batches of 3, 3 and 1"""
    x = sm.stream('tones')
    with chan(max_blocks=3, host_out=True) as ch:
        ch.survey_start(log2n)
        for r in reads(x):
            ch.push(r)
        ch.run()
        equal(ch.survey_read(), sm.reference('tones', log2n), 'log2n %d' % log2n)
        assert ch.stat('survey_launches') == 2 * 3


def test_device_push(engine_lib):
    import torch
    x = sm.stream('tones')
    t = torch.from_numpy(np.array(x).view(np.float32)).to('cuda')
    torch.cuda.synchronize()
    with chan(max_blocks=2) as ch:
        ch.survey_start(13)
        for b in range(0, 6, 2):
            ch.push_device(t.data_ptr() + b * B * 8, 2)
            ch.run()
        ch.push_device(t.data_ptr() + 6 * B * 8, 1)
        ch.run()
        equal(ch.survey_read(), sm.reference('tones', 13), 'push_device')


@pytest.mark.parametrize('window', ['none', 'hann', 'odd'])
@pytest.mark.parametrize('log2n', [12, 14])
def test_windows(engine_lib, window, log2n):
    x = sm.stream('tones')
    with chan(max_blocks=2) as ch:
        ch.survey_start(log2n, sm.WINDOWS[window](1 << log2n))
        for b in range(0, 7, 2):
            ch.push(x[b * B:(b + 2) * B])
            ch.run()
        equal(ch.survey_read(), sm.reference('tones', log2n, window), '%s %d' % (window, log2n))


def test_hann_by_name_is_the_numpy_window(engine_lib):
    x = sm.stream('tones')
    with chan() as ch:
        ch.survey_start(12, 'hann')
        one_read_per_run(ch, x)
        equal(ch.survey_read(), sm.reference('tones', 12, 'hann'), "'hann'")


@pytest.mark.parametrize('kind', ['zeros', 'fullscale', 'tailpulse'])
@pytest.mark.parametrize('log2n', [12, 13, 14])
def test_input_classes(engine_lib, kind, log2n):
    import aero_engine as ae
    x = sm.stream(kind)
    want = sm.reference(kind, log2n)
    with chan() as ch:
        ch.survey_start(log2n)
        one_read_per_run(ch, x)
        got = ch.survey_read()
        equal(got, want, '%s %d' % (kind, log2n))
    if kind == 'zeros':
        assert not got[0].view(np.uint64).any()  # exactly +0
        assert ae.survey_peaks(got[0], log2n, FS, C) == []
    elif kind == 'tailpulse':  # the pulse lies in one segment: a flat spectrum of |pulse|^2
        assert np.all(got[0] > 0) and np.allclose(got[0], 0.75 ** 2 + 0.5 ** 2, rtol=1e-12)
    else:
        assert np.count_nonzero(got[0]) > got[0].size // 2


def test_dc_removal(engine_lib):
    """correct_dc_bias: the survey sees the stream after dc_kernel"""
    x = sm.stream('dc', nreads=3)
    with chan(max_blocks=2, dcc=True) as ch:
        ch.survey_start(12)
        ch.push(x[:2 * B])
        ch.run()
        ch.push(x[2 * B:])
        ch.run()
        got = ch.survey_read()
    equal(got, sm.reference('dc', 12, nreads=3, dcc=True), 'dc')
    raw = sm.reference('dc', 12, nreads=3)
    assert got[0][0] < raw[0][0]  # bin 0 lost some of the offset's power


def test_reset_in_mid_stream_and_restart(engine_lib):
    x = sm.stream('tones')
    m = sm.SurveyModel(13)
    with chan() as ch:
        ch.survey_start(13)
        one_read_per_run(ch, x[:3 * B])
        m.feed(x[:3 * B])
        equal(ch.survey_read(reset=True), m.read(reset=True), 'first half')
        equal(ch.survey_read(), (np.zeros(8192), 0), 'after the reset')
        one_read_per_run(ch, x[3 * B:5 * B])
        m.feed(x[3 * B:5 * B])  # the tail of read 3 goes on: the grid is not reset
        equal(ch.survey_read(), m.read(), 'second half')
        assert ch.stat('survey_segments') == m.total
        # stop and start: a fresh grid at the next read, the old tail is gone
        ch.survey_stop()
        import aero_engine as ae
        with pytest.raises(ae.AeroError):
            ch.survey_read()
        with pytest.raises(ae.AeroError):
            ch.survey_stop()
        ch.survey_start(12)
        with pytest.raises(ae.AeroError):
            ch.survey_start(12)
        one_read_per_run(ch, x[5 * B:])
        equal(ch.survey_read(), sm.survey(x[5 * B:], 12), 'restarted')
        for bad in (11, 15, 0):
            ch.survey_stop()
            with pytest.raises(ae.AeroError):
                ch.survey_start(bad)
            ch.survey_start(12)


def test_start_after_two_reads(engine_lib):
    """segment 0 begins at read 2, also when read 1 is pushed and not yet run at the start"""
    x = sm.stream('tones')
    with chan(max_blocks=2) as ch:
        ch.push(x[:B])
        ch.run()
        ch.push(x[B:2 * B])
        ch.survey_start(14)  # runs read 1 without the survey
        one_read_per_run(ch, x[2 * B:])
        equal(ch.survey_read(), sm.survey(x[2 * B:], 14), 'late start')


def _audio_equal(ch, ref, cfg, what):
    for v in range(len(cfg['vfos'])):
        want, got = ref.usb(v), ch.audio(v)
        assert len(want) > 0 and np.array_equal(want, got), '%s: audio of vfo %d' % (what, v)
    for m in range(len(cfg['mains'])):
        assert np.array_equal(ref.iq(m), ch.iq(m)), '%s: IQ of main %d' % (what, m)


@pytest.mark.parametrize('dcc', [False, True])
def test_audio_does_not_change(engine_lib, dcc):
    """a survey that starts and stops in mid-stream: every VFO's audio is the oracle publisher's"""
    x = sm.stream('dc' if dcc else 'tones', nreads=5 if dcc else 7)
    ref = tl.OraclePublisher(FS, C, CFG['mains'], CFG['vfos'], correct_dc_bias=dcc)
    ref.process(x)
    nr = len(x) // B
    seen = (sm.dc_remove(x) if dcc else x)[B:(nr - 2) * B]  # reads 1 .. nr-3, the DC state from read 0
    with chan(max_blocks=2, host_out=True, dcc=dcc) as ch:
        for b, r in enumerate(reads(x)):
            if b == 1:
                ch.survey_start(12, 'hann')  # runs read 0 without it
            if b == nr - 2:
                ch.run()
                equal(ch.survey_read(), sm.survey(seen, 12, sm.hann(4096)), 'reads 1 .. %d' % (nr - 3))
                ch.survey_stop()
            ch.push(r)
        ch.run()
        ch.sync()
        assert ch.stat('survey_launches') > 0
        _audio_equal(ch, ref, CFG, 'survey on')
    with chan(max_blocks=2, host_out=True, dcc=dcc) as ch:  # and none at all
        for r in reads(x):
            ch.push(r)
        ch.run()
        ch.sync()
        assert ch.stat('survey_launches') == 0 and ch.stat('survey_segments') == 0
        _audio_equal(ch, ref, CFG, 'no survey')


def test_vfos_come_and_go(engine_lib):
    x = sm.stream('tones')
    with chan(max_blocks=2) as ch:
        ch.survey_start(13)
        one_read_per_run(ch, x[:2 * B])
        ch.push(x[2 * B:3 * B])
        v = ch.open_vfo(dict(frequency=C - 20000, data_rate=1200, gain=100.0))  # runs read 2
        one_read_per_run(ch, x[3 * B:5 * B])
        ch.close_vfo(0)
        ch.skip_vfo(v, True)
        one_read_per_run(ch, x[5 * B:])
        equal(ch.survey_read(), sm.reference('tones', 13), 'open / close / skip')


def test_second_read_length(engine_lib):
    """1.536 Msps: reads of 384000 samples, 23.4 segments of 16384 each, a longer scratch"""
    cfg = tl.PUB_CONFIGS['r1536k']
    x = sm.stream('tones', 1536000, 2, 384000)
    with chan(max_blocks=2, cfg=cfg) as ch:
        assert ch.block_len == 384000
        ch.survey_start(14)
        ch.push(x[:384000])
        ch.run()
        ch.push(x[384000:])
        ch.run()
        equal(ch.survey_read(), sm.reference('tones', 14, 'none', 1536000, 2, 384000), 'r1536k')
