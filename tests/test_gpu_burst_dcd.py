"""AeroL's 1 s DCD timer on burst channels (AERO_F_DCD_TICK_BURST) on the GPU
against the oracle with the timer slot run between messages
(tests/oracle_tick.py): the tick of sample 48000 k - 1 fires at the end of the
message that holds it.  Delivered soft bits, trident records (f64 bits), every
R/T test, every packet, the ACARS items and the DataCarrierDetect changes must
be identical, through every push path, across aero_run boundaries, a channel
move and a slot reuse; and each OQPSK case differs from the untimed oracle in
its R/T tests, so it cannot pass with the tick ignored."""
import functools

import numpy as np
import pytest

import aero_testlib as tl
import oracle_tick as ot

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _pcm(seconds, seed, db):
    return tl.synth_burst(seconds=float(seconds), seed=seed, carrier=12000.0, ebn0=db)


@functools.lru_cache(maxsize=None)
def _msk_pcm():
    return tl.synth_burst_msk(seconds=20.0, bitrate=1200, seed=0xAE70)


@functools.lru_cache(maxsize=None)
def _ref(seconds, seed, db, size, tick=True):
    """the oracle's outputs for the stream in `size`-sample messages; computed once, never changed"""
    return ot.run(_pcm(seconds, seed, db), size, tick=tick)


@functools.lru_cache(maxsize=None)
def _msk_ref(size, tick=True):
    return ot.run(_msk_pcm(), size, bitrate=1200, tick=tick)


def _flags(ae, tick=True):
    return ae.F_TRACE_SOFT | ae.F_TRACE_HOPS | ae.F_TRACE_FRAMES | (ae.F_DCD_TICK_BURST if tick else 0)


def _take(eng, ch):
    return dict(soft=eng.softbits16(ch), hops=eng.hops(ch), tests=eng.rt_tests(ch), packets=eng.rt_packets(ch),
                items=eng.items(ch), edges=eng.channel_events(ch)[0])


def _join(a, b):
    out = {k: (a[k] + b[k]) if isinstance(a[k], list) else np.concatenate([a[k], b[k]]) for k in a if k != 'edges'}
    out['edges'] = b['edges']  # the counter travels with the channel
    return out


def _equal(got, ref, what=''):
    assert len(ref['soft']) > 1000, 'the oracle did not lock'
    assert len(got['soft']) == len(ref['soft']) and np.array_equal(got['soft'], ref['soft']), '%s soft bits' % what
    assert got['hops'].shape == ref['hops'].shape and \
        np.array_equal(got['hops'].view(np.int64), ref['hops'].view(np.int64)), '%s trident records' % what
    assert np.array_equal(got['tests'], ref['tests']), '%s R/T tests' % what
    assert got['packets'] == ref['packets'], '%s R/T packets' % what
    assert got['items'] == ref['items'], '%s items' % what
    assert got['edges'] == ref['edges'], '%s DCD changes' % what


def _feed(eng, ch, msgs, every, first=0):
    """pushes msgs, aero_run after every `every`-th; the events are read after
    aero_run + aero_sync (the last message's tick has no successor)"""
    for k, m in enumerate(msgs, first):
        eng.push(ch, m)
        if (k + 1) % every == 0:
            eng.run()
    eng.run()
    eng.sync()


@pytest.mark.parametrize('seconds,seed,db,size,every', [(20, 2, 14.0, 4800, 1), (20, 0xAE50, 12.0, 7000, 3),
                                                        (12, 7, 10.0, 12000, 2)])
def test_ticked_channel_equals_hook_oracle(engine_lib, seconds, seed, db, size, every):
    """ticks on run boundaries, between the queued messages of one run (with
    messages that do not divide 48000), and on the last message of a run"""
    import aero_engine as ae
    ref, untimed = _ref(seconds, seed, db, size), _ref(seconds, seed, db, size, False)
    assert not np.array_equal(ref['tests'], untimed['tests']), 'the stream does not tell the timer'
    eng = ae.Engine(max_channels=1, flags=_flags(ae))
    ch = eng.open_channel(10500, 48000, burst=True)
    _feed(eng, ch, ot.messages(_pcm(seconds, seed, db), size), every)
    got = _take(eng, ch)
    eng.close()
    _equal(got, ref)
    assert not np.array_equal(got['tests'], untimed['tests'])


def test_ticked_batch_push_equals_hook_oracle(engine_lib):
    """aero_push_pcm_batch, host and device pointers in turn: the device
    counts each message's ticks as the host does"""
    import aero_engine as ae
    import torch
    keys, size = [(20, 2, 14.0), (20, 7, 10.0), (20, 0xAE50, 12.0)], 12000
    x = np.stack([_pcm(*k) for k in keys], axis=1)  # time-major [L][3]
    L, n = x.shape
    assert L % size == 0
    eng = ae.Engine(max_channels=n, flags=_flags(ae))
    chans = [eng.open_channel(10500, 48000, burst=True) for _ in range(n)]
    assert chans == list(range(n))
    xd = torch.from_numpy(x).to('cuda')
    torch.cuda.synchronize()
    for k, t in enumerate(range(0, L, size)):
        if k % 2:
            eng.push_batch(x[t:t + size])
        else:
            eng.push_batch_device(xd[t:].data_ptr(), size, n, n)
        eng.run()
    eng.sync()
    got = [_take(eng, ch) for ch in chans]
    eng.close()
    for k, key in enumerate(keys):
        _equal(got[k], _ref(*key, size), 'channel %d:' % k)


def test_continuous_flag_leaves_burst_channels_untimed(engine_lib):
    """AERO_F_DCD_TICK alone (what bench.py sets on its burst engines): burst channels ignore it"""
    import aero_engine as ae
    eng = ae.Engine(max_channels=1, flags=_flags(ae, tick=False) | ae.F_DCD_TICK)
    ch = eng.open_channel(10500, 48000, burst=True)
    _feed(eng, ch, ot.messages(_pcm(20, 2, 14.0), 4800), 1)
    got = _take(eng, ch)
    eng.close()
    _equal(got, _ref(20, 2, 14.0, 4800, False))


def test_ticked_channel_moves_between_engines(engine_lib):
    """exported after 10 s with its last message (which completes a second:
    its tick is counted, not yet recorded) pushed and not run; the sample count
    since open, the countdown and the tick rings travel in the blob"""
    import aero_engine as ae
    msgs = ot.messages(_pcm(20, 2, 14.0), 4800)
    src = ae.Engine(max_channels=2, flags=_flags(ae))
    ch = src.open_channel(10500, 48000, burst=True)
    _feed(src, ch, msgs[:99], 1)
    src.push(ch, msgs[99])
    blob = src.export_channel(ch)
    first = _take(src, ch)
    src.close_channel(ch)
    plain = ae.Engine(max_channels=2, flags=_flags(ae, tick=False))
    with pytest.raises(ae.AeroError) as err:
        plain.import_channel(blob)
    assert err.value.rc == ae.AERO_E_INVALID
    plain.close()
    dst = ae.Engine(max_channels=70, flags=_flags(ae))  # another column pitch
    dst.open_channel(10500, 48000, burst=True)         # and another slot
    moved = dst.import_channel(blob)
    _feed(dst, moved, msgs[100:], 1, first=100)
    got = _join(first, _take(dst, moved))
    src.close()
    dst.close()
    _equal(got, _ref(20, 2, 14.0, 4800))


def test_ticked_burst_msk(engine_lib):
    """burst MSK does not gate its sync on datacd: the timer adds DataCarrierDetect changes only"""
    import aero_engine as ae
    ref = _msk_ref(4800)
    assert ref['edges'] == 4 and _msk_ref(4800, False)['edges'] == 1
    eng = ae.Engine(max_channels=1, flags=_flags(ae))
    ch = eng.open_channel(1200, 48000, burst=True)
    _feed(eng, ch, ot.messages(_msk_pcm(), 4800), 1)
    got = _take(eng, ch)
    eng.close()
    assert got['edges'] == 4
    _equal(got, ref)


def test_reopened_slot_starts_a_fresh_timer(engine_lib):
    """closed after a sync and before its fourth tick (datacd set, the
    countdown running, ticks counted since open), the slot reopened: the new
    channel equals a fresh ticked oracle"""
    import aero_engine as ae
    pcm = _pcm(20, 2, 14.0)
    msgs = ot.messages(pcm, 4800)
    # the first message after which datacd is set and a tick has since fired without clearing it
    o = ot.TickOracle()
    stop = None
    for k, m in enumerate(msgs):
        before, ticks = o.events()[0], o.ticks
        o.push(m)
        if before % 2 == 1 and o.events()[0] == before and o.ticks > ticks:
            stop = k + 1
            break
    assert stop is not None and 0 < stop < len(msgs)
    eng = ae.Engine(max_channels=1, flags=_flags(ae))
    ch = eng.open_channel(10500, 48000, burst=True)
    _feed(eng, ch, msgs[:stop], 1)
    assert eng.channel_events(ch)[0] % 2 == 1, 'datacd is not set at the close'
    resets = eng.stat('slot_resets')
    eng.close_channel(ch)
    again = eng.open_channel(10500, 48000, burst=True)
    assert again == ch
    _feed(eng, again, msgs, 1)
    assert eng.stat('slot_resets') == resets + 1
    got = _take(eng, again)
    eng.close()
    _equal(got, _ref(20, 2, 14.0, 4800))
