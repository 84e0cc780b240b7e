"""The message-boundary paths of the 8400-bps C channel and of burst channels.

The C channel's prefilter runs once per message and a burst message is one
writeDataSlot call, so their output depends on where the pushed messages are
cut.  Every way a message end reaches the engine is run here against tl.Oracle
fed the same messages in the same order, bit for bit: several messages queued
on a channel before one aero_run (channels of one engine at different queue
depths, the early pass inside a push that would overrun the PCM ring, more
queued messages than one gather-job table holds), aero_push_pcm_dev mixed with
host pushes, the three variants of aero_push_pcm_batch, the channeliser's
aero_chan_feed with one, two and three reads per batch (each read is one
message, publish/vfo.cpp:184), and an export with messages pending.

No case is vacuous: each asserts that the oracle alone decoded frames, SUs and
voice frames (tl.c_produced) or R/T packets; tests/test_msg_boundaries.py
checks the same on the CPU, and that the streams tell the message cuts apart."""
import concurrent.futures as cf

import numpy as np
import pytest

import aero_testlib as tl
import oracle_tick as ot

pytestmark = pytest.mark.gpu

# 6-s C streams (seed, carrier Hz); the 64 channels of the batch cases carry them in turn
STREAMS = [(0xC1A5, 11000.0), (0xC1A7, 12037.5), (0xC1A8, 9050.0), (0xC1A9, 14000.0)]
B_STREAM = (0xC1A6, 12000.0)
B_TINY = 4100  # messages of 3 samples: more than the 4096 gather jobs of one table

# Case A, per channel: stream, message sizes, messages queued before each
# aero_run (cycled).  In one round the channels stand at different depths; 5
# messages of 12000 fit the 65536-sample ring, 7 do not (the sixth push runs a
# pass first); the ragged list is queued four at a time.
A_PLAN = [(0, (12000,), (1, 3, 0, 2, 5, 7, 0)),
          (1, tl.RAGGED, (4, 0, 4, 4, 0, 4, 4)),
          (2, (12000,), (0, 7, 2, 0, 5, 1, 3))]


def _stream(k):
    seed, carrier = STREAMS[k]
    return tl.synth_c(seconds=6.0, seed=seed, carrier=carrier, ebn0=12.0)


def b_messages():
    pcm = tl.synth_c(seconds=6.0, seed=B_STREAM[0], carrier=B_STREAM[1], ebn0=12.0)
    tiny = [pcm[3 * i:3 * i + 3] for i in range(B_TINY)]
    return tiny + tl.cut(pcm[3 * B_TINY:], (12000,))


def build_refs():
    """every C-channel oracle of this module, computed once: (stream, 'ragged'
    or 12000) -> outputs, and 'B'"""
    jobs = {(k, 'ragged'): tl.cut(_stream(k), tl.RAGGED) for k in range(len(STREAMS))}
    jobs.update({(k, 12000): tl.cut(_stream(k), (12000,)) for k in (0, 2)})
    jobs['B'] = b_messages()
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        futs = {key: ex.submit(tl.c_reference, m) for key, m in jobs.items()}
        return {key: f.result() for key, f in futs.items()}


@pytest.fixture(scope='module')
def refs(cpu_libs):
    return build_refs()


@pytest.fixture(scope='module')
def feed_refs(cpu_libs):
    """case E: the oracle publisher's audio, one read per message, through the oracle decoders"""
    x, audio, block_len, spb = tl.boundary_input()
    return dict(x=x, block_len=block_len, spb=spb, c=tl.c_reference(tl.cut(audio[0], (spb[0],))),
                burst=ot.run(audio[1], spb[1], tick=True))


def _all_traces(ae):
    return ae.F_TRACE_PT | ae.F_TRACE_SOFT | ae.F_TRACE_HOPS | ae.F_TRACE_FRAMES


# ------------------------------------------------------------------ A
@pytest.mark.parametrize('order', ['immediate', 'deferred'])
def test_queued_messages(engine_lib, refs, order):
    """A: three C channels, several messages per channel before each aero_run,
    with the trace flags (each pass's Viterbi at once) and with
    F_TRACE_FRAMES alone (a pass's Viterbi inside the next pass)"""
    import aero_engine as ae
    eng = ae.Engine(max_channels=3, flags=_all_traces(ae) if order == 'immediate' else ae.F_TRACE_FRAMES)
    chans = [eng.open_channel(8400, 48000) for _ in A_PLAN]
    msgs = [tl.cut(_stream(s), sizes) for s, sizes, _ in A_PLAN]
    pos, r, seen = [0] * len(A_PLAN), 0, set()
    while any(p < len(m) for p, m in zip(pos, msgs)):
        depth = [min(A_PLAN[k][2][r % len(A_PLAN[k][2])], len(msgs[k]) - pos[k]) for k in range(len(A_PLAN))]
        for j in range(max(depth)):  # the channels' messages interleaved in one queue
            for k, ch in enumerate(chans):
                if j < depth[k]:
                    eng.push(ch, msgs[k][pos[k]])
                    pos[k] += 1
        seen.update((k, d) for k, d in enumerate(depth))
        eng.run()
        r += 1
    eng.flush()
    eng.sync()
    assert {(0, 2), (0, 5), (0, 7), (2, 7), (1, 4), (2, 0)} <= seen, 'the plan lost a queue depth'
    for k, ch in enumerate(chans):
        ref = refs[(A_PLAN[k][0], 'ragged' if A_PLAN[k][1] is tl.RAGGED else 12000)]
        tl.c_equal(tl.c_take(eng, ch), ref, 'channel %d' % k, ('soft', 'pt', 'hops') if order == 'immediate' else ())
    eng.close()


# ------------------------------------------------------------------ B
def test_more_queued_messages_than_gather_jobs(engine_lib, refs):
    """B: 4100 three-sample messages queued on one channel (the host queue
    flushes at 4096 gather jobs), one aero_run, then the rest of the stream"""
    import aero_engine as ae
    msgs = b_messages()
    eng = ae.Engine(max_channels=1, flags=_all_traces(ae))
    ch = eng.open_channel(8400, 48000)
    for m in msgs[:B_TINY]:
        eng.push(ch, m)
    eng.run()
    for m in msgs[B_TINY:]:
        eng.push(ch, m)
        eng.run()
    eng.flush()
    eng.sync()
    tl.c_equal(tl.c_take(eng, ch), refs['B'], 'channel 0')
    eng.close()


# ------------------------------------------------------------------ C
def test_device_pushes_between_host_pushes(engine_lib, refs):
    """C: aero_push_pcm_dev; channel 0 takes host and device messages in turn
    (ring writes and counters stay in push order), channel 1 device messages
    only; ragged sizes, two or three messages per aero_run"""
    import torch
    import aero_engine as ae
    streams = [_stream(0), _stream(1)]
    msgs = [tl.cut(s, tl.RAGGED) for s in streams]
    dev = [torch.from_numpy(s).to('cuda') for s in streams]
    torch.cuda.synchronize()
    eng = ae.Engine(max_channels=2, flags=_all_traces(ae))
    chans = [eng.open_channel(8400, 48000) for _ in streams]
    off, i, r = [0, 0], 0, 0
    while i < len(msgs[0]):
        for _ in range(min(2 + r % 2, len(msgs[0]) - i)):
            for k, ch in enumerate(chans):
                m = msgs[k][i]
                if k == 0 and i % 2 == 0:
                    eng.push(ch, m)
                else:
                    eng.push_device(ch, dev[k].data_ptr() + 2 * off[k], len(m))
                off[k] += len(m)
            i += 1
        eng.run()
        r += 1
    eng.flush()
    eng.sync()
    for k, ch in enumerate(chans):
        tl.c_equal(tl.c_take(eng, ch), refs[(k, 'ragged')], 'channel %d' % k)
    eng.close()


# ------------------------------------------------------------------ D
@pytest.mark.parametrize('source,nch', [('pageable', 4), ('pinned', 64), ('device', 64)])
def test_batch_pushes(engine_lib, refs, source, nch):
    """D: aero_push_pcm_batch, one message per channel per call on the ragged
    schedule, every second round two calls before the aero_run: a pageable
    host array, a pinned one (64 channels: whole ring rows, the 1-D DMA) and a
    device pointer"""
    import torch
    import aero_engine as ae
    x = np.ascontiguousarray(np.stack([_stream(k % 4) for k in range(nch)], axis=1))  # time-major [L][nch]
    L = x.shape[0]
    if source == 'pinned':
        t = torch.from_numpy(x).pin_memory()
    elif source == 'device':
        t = torch.from_numpy(x).to('cuda')
        torch.cuda.synchronize()
    eng = ae.Engine(max_channels=nch, flags=ae.F_TRACE_SOFT | ae.F_TRACE_HOPS | ae.F_TRACE_FRAMES)
    assert [eng.open_channel(8400, 48000) for _ in range(nch)] == list(range(nch))
    p, i, r = 0, 0, 0
    while p < L:
        for _ in range(1 + r % 2):
            n = min(tl.RAGGED[i % len(tl.RAGGED)], L - p)
            if n == 0:
                break
            if source == 'pageable':
                eng.push_batch(x[p:p + n])
            elif source == 'pinned':
                eng.push_batch_host(t.data_ptr() + 2 * nch * p, n, nch, nch)
            else:
                eng.push_batch_device(t.data_ptr() + 2 * nch * p, n, nch, nch)
            p += n
            i += 1
        eng.run()
        r += 1
    eng.flush()
    eng.sync()
    for k in range(nch):
        traces = ('soft', 'hops') if k in (0, 1, nch - 2, nch - 1) else ()
        tl.c_equal(tl.c_take(eng, k), refs[(k % 4, 'ragged')], 'channel %d' % k, traces)
    eng.close()


# ------------------------------------------------------------------ E
def test_channeliser_feed_is_one_message_per_read(engine_lib, feed_refs):
    """E: a 288-kHz channeliser feeds a C channel and a burst OQPSK channel
    (with its DCD timer) through aero_chan_feed, one, two and three reads per
    batch in turn; expected: the oracle publisher's audio pushed into the
    oracle decoders one read per message, whatever the batch held"""
    import aero_engine as ae
    cfg, x, B = tl.BOUNDARY_CFG, feed_refs['x'], feed_refs['block_len']
    assert len(feed_refs['burst']['packets']) >= 2, 'the burst oracle decoded too little'
    ch = ae.Channeliser(cfg['sample_rate'], cfg['center_frequency'], cfg['mains'], cfg['vfos'], max_blocks=3)
    assert ch.block_len == B
    assert [ch.vfo_info(v)['samples_per_block'] for v in range(2)] == feed_refs['spb']
    eng = ae.Engine(max_channels=2, flags=_all_traces(ae) | ae.F_DCD_TICK_BURST)
    chans = [eng.open_channel(8400, 48000), eng.open_channel(10500, 48000, burst=True)]
    nblk, b, r, seen = len(x) // B, 0, 0, set()
    while b < nblk:
        k = min(1 + r % 3, nblk - b)
        ch.push(x[b * B:(b + k) * B])
        ch.run()
        ch.feed(eng, chans)
        eng.run()
        seen.add(k)
        b += k
        r += 1
    assert seen == {1, 2, 3}
    eng.flush()
    eng.sync()
    tl.c_equal(tl.c_take(eng, chans[0]), feed_refs['c'], 'the C channel')
    got, ref = chans[1], feed_refs['burst']
    soft = eng.softbits16(got)
    assert len(ref['soft']) > 1000 and len(soft) == len(ref['soft']) and np.array_equal(soft, ref['soft']), \
        'the burst channel: soft bits'
    h = eng.hops(got)
    assert h.shape == ref['hops'].shape and np.array_equal(h.view(np.int64), ref['hops'].view(np.int64)), \
        'the burst channel: trident records'
    assert np.array_equal(eng.rt_tests(got), ref['tests']), 'the burst channel: R/T tests'
    assert eng.rt_packets(got) == ref['packets'], 'the burst channel: R/T packets'
    assert eng.channel_events(got)[0] == ref['edges'], 'the burst channel: DCD changes'
    eng.close()
    ch.close()


# ------------------------------------------------------------------ F
def test_export_with_messages_pending(engine_lib, refs):
    """F: three ragged C messages pushed and not run at aero_channel_export;
    the source's output followed by the destination's equals the uninterrupted oracle"""
    import aero_engine as ae
    msgs = tl.cut(_stream(3), tl.RAGGED)
    # 4.26 s in (the oracle has delivered two frames, three are to come); the
    # pending messages end just before, on and just past a prefilter block
    split = 27
    assert sum(len(m) for m in msgs[:split]) == 204603
    assert [len(m) for m in msgs[split:split + 3]] == [2047, 2048, 2049]
    A = ae.Engine(max_channels=64, flags=_all_traces(ae))
    B = ae.Engine(max_channels=128, flags=_all_traces(ae))  # another column pitch
    src = A.open_channel(8400, 48000)
    B.open_channel(8400, 48000)  # and another slot
    for m in msgs[:split]:
        A.push(src, m)
        A.run()
    for m in msgs[split:split + 3]:
        A.push(src, m)
    blob = A.export_channel(src)
    head = tl.c_take(A, src)
    A.close_channel(src)
    dst = B.import_channel(blob)
    assert dst == 1
    B.run()
    for m in msgs[split + 3:]:
        B.push(dst, m)
        B.run()
    B.flush()
    B.sync()
    tail = tl.c_take(B, dst)
    assert len(head['frames']) >= 320 and len(tail['frames']) >= 320, 'the split does not fall between two frames'
    got = {k: (head[k] + tail[k]) if isinstance(head[k], list) else np.concatenate([head[k], tail[k]])
           for k in head if k != 'edges'}
    got['edges'] = tail['edges']  # the counter travels with the channel
    tl.c_equal(got, refs[(3, 'ragged')], 'the moved channel')
    A.close()
    B.close()
