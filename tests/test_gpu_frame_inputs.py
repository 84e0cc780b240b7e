"""The framing kernels, the Viterbi's post step, process_slot's host assembly
and PChannelHost on the adversarial frame content of tests/frame_inputs.py
(tests/test_frame_inputs.py proves on the CPU what each class reaches),
against the oracle: soft bits, Viterbi blocks, frame records (bytes, length,
CRC mask), items with reassembly on and off and the DataCarrierDetect changes
must all be equal, without a tolerance.

The classes of a kind are the channels of one engine (each twice: reassembly
on and off), so a resyncing lane, a flywheel lane and a clean lane share a
wave and a Viterbi batch.  What a channel has delivered after a run() is a
prefix of the oracle's output (a pass's Viterbi may run inside the next pass,
and a channel stopped at a tick resumes a pass later); after flush() it is
equal."""
import numpy as np
import pytest

import aero_testlib as tl
import frame_inputs as fi

pytestmark = pytest.mark.gpu

KEYS = ('soft', 'blocks', 'frames', 'items', 'fragments')


def compare(got, ref, what, final=True):
    """got: what a channel pair delivered so far; equal to the oracle's at the
    end, a prefix of it before"""
    for k in KEYS:
        if k not in got:
            continue
        g, r = got[k], ref[k]
        if final:
            assert len(g) == len(r), '%s: %d %s, the oracle %d' % (what, len(g), k, len(r))
        else:
            assert len(g) <= len(r), '%s: more %s than the oracle' % (what, k)
        same = (g == r[:len(g)]) if isinstance(g, list) else np.array_equal(g, r[:len(g)])
        assert same, '%s: %s differ' % (what, k)
    if final:
        assert got['edges'] == ref['edges'], '%s: DCD changes %d, the oracle %d' % (what, got['edges'], ref['edges'])
    else:
        assert got['edges'] <= ref['edges'], '%s: more DCD changes than the oracle' % what


def altered(kind, name, good):
    """references that are wrong in one decision of the class (the CPU test
    tests/test_frame_inputs.py shows that compare() tells them from the oracle's)"""
    out = []
    if name == 'crc_zero':  # one mask bit of an all-zero SU
        fr = good['frames'].copy().reshape(-1, 320)
        k = next(i for i, (f, m) in enumerate(tl.frame_records(fr)) if fi.ZERO_SU in [f[j:j + 12] for j in range(0, len(f), 12)])
        f = tl.frame_records(fr)[k][0]
        su = [f[j:j + 12] for j in range(0, len(f), 12)].index(fi.ZERO_SU)
        fr[k, 316 + su // 8] ^= 1 << (su % 8)
        out.append(dict(good, frames=fr.reshape(-1)))
    elif name == 'crc_mix':  # one countdown step: the tick that takes 2 to -1 left out
        s = fi.stream(kind, name)
        compare(fi.run_oracle(kind, s.pcm, skip_tick=-1), good, 'every tick fired')  # the hooked oracle is the oracle
        out.append(fi.run_oracle(kind, s.pcm, skip_tick=fi.mix_skip(kind, s)))
    else:  # the clear decision: the broken frame's blocks left in the next record
        fr = good['frames'].copy().reshape(-1, 320)
        lens = fr[:, 312:316].copy().view(np.uint32).reshape(-1)
        k = int(np.nonzero(lens == 72)[0][-3])
        fr[k, 312] = 72 + 24
        out.append(dict(good, frames=fr.reshape(-1)))
    return out


def _flags(ae, kind, tick, traced):
    f = ae.F_TRACE_FRAMES
    if traced:
        f |= ae.F_TRACE_SOFT | ae.F_TRACE_BLOCKS
    if tick:
        f |= ae.F_DCD_TICK if kind == 'p10500' else ae.F_DCD_TICK_CONT
    return f


def _take(eng, pair, acc, traced):
    on, off = pair
    if traced:
        acc['soft'] = np.concatenate([acc['soft'], eng.softbits(on)])
        acc['blocks'] = np.concatenate([acc['blocks'], eng.blocks(on)])
    acc['frames'] = np.concatenate([acc['frames'], eng.frames(on)])
    acc['items'] += eng.items(on)
    acc['fragments'] += eng.items(off)
    acc['edges'] = eng.channel_events(on)[0]
    # the twin differs in its host's reassembly alone
    acc['twin_frames'] = np.concatenate([acc['twin_frames'], eng.frames(off)])
    acc['twin_edges'] = eng.channel_events(off)[0]


def _new_acc(traced):
    e = np.zeros(0, np.uint8)
    acc = dict(frames=e, items=[], fragments=[], edges=0, twin_frames=e, twin_edges=0)
    if traced:
        acc.update(soft=e, blocks=e)
    return acc


def _run(kind, schedule, tick, traced=True, names=None):
    import aero_engine as ae
    K = fi.KINDS[kind]
    names = list(names or fi.classes(kind))
    refs = [fi.reference(kind, n, schedule, tick) for n in names]
    eng = ae.Engine(max_channels=2 * len(names), flags=_flags(ae, kind, tick, traced))
    pairs = [(eng.open_channel(K['bitrate'], fs=K['fs']), eng.open_channel(K['bitrate'], fs=K['fs'], disable_reassembly=True))
             for _ in names]
    msgs = [fi.messages(len(fi.stream(kind, n).pcm), schedule) for n in names]
    accs = [_new_acc(traced) for _ in names]
    for k in range(max(len(m) for m in msgs)):
        for n, pair, m in zip(names, pairs, msgs):
            if k < len(m):
                pcm = fi.stream(kind, n).pcm[m[k][0]:m[k][1]]
                for ch in pair:
                    eng.push(ch, pcm)
        eng.run()
        for n, pair, acc, ref in zip(names, pairs, accs, refs):
            _take(eng, pair, acc, traced)
            compare(acc, ref, '%s %s run %d' % (kind, n, k), final=False)
    eng.flush()
    for n, pair, acc, ref in zip(names, pairs, accs, refs):
        _take(eng, pair, acc, traced)
        compare(acc, ref, '%s %s' % (kind, n))
        assert np.array_equal(acc['twin_frames'], ref['frames']) and acc['twin_edges'] == ref['edges'], n
    eng.close()


@pytest.mark.parametrize('order', ['traced', 'frames'])
@pytest.mark.parametrize('tick', [False, True], ids=['untimed', 'tick'])
@pytest.mark.parametrize('schedule', fi.SCHEDULES)
def test_p10500(engine_lib, cpu_libs, oqpsk_kernel, schedule, tick, order):
    """`order`: with the soft trace a pass's Viterbi runs right after its
    framing; frames-only it runs inside the next pass (the production order)"""
    _run('p10500', schedule, tick, traced=order == 'traced')


@pytest.mark.parametrize('tick', [False, True], ids=['untimed', 'tick'])
@pytest.mark.parametrize('schedule', fi.SCHEDULES)
@pytest.mark.parametrize('kind', ['msk600', 'msk1200'])
def test_msk(engine_lib, cpu_libs, msk_kernel, kind, schedule, tick):
    _run(kind, schedule, tick)


@pytest.mark.parametrize('kind', ['p10500', 'msk600'])
def test_partial_second_wave(engine_lib, cpu_libs, kind):
    """the classes repeated to 70 channels: a partial second wave of the framing kernel"""
    names = fi.classes(kind)
    names = (names * (35 // len(names) + 1))[:35]
    _run(kind, '12000', True, traced=False, names=names)


@pytest.mark.parametrize('kind', ['p10500', 'msk600'])
def test_export_import_mid_stream(engine_lib, cpu_libs, kind):
    """Every channel is exported and imported into another engine between the
    adversarial frames, where a timer class has datacd down and the ISU classes
    hold ISUs whose SSUs are still to come; the moved channels continue bit for bit."""
    import aero_engine as ae
    K = fi.KINDS[kind]
    names = list(fi.classes(kind))
    tick = True
    refs = [fi.reference(kind, n, '12000', tick) for n in names]
    # the first message inside the adversarial part before and after which the oracle has datacd down
    # (an even count of changes) on one of the timer's classes: the export falls between the two
    s0 = fi.stream(kind, names[0])
    steps = {n: [e for _, _, e in r['steps']] for n, r in zip(names, refs)}
    first = s0.adv_sample // 12000 + 1
    at = next((k for k in range(first, len(steps[names[0]]) - 2)
               if any(n in fi.TICK_CLASSES and k < len(steps[n]) and steps[n][k - 1] % 2 == 0 and steps[n][k] % 2 == 0
                      for n in names)), None)
    assert at is not None, 'no class has datacd down inside the adversarial part'
    flags = _flags(ae, kind, tick, True)
    A = ae.Engine(max_channels=len(names), flags=flags)
    B = ae.Engine(max_channels=3 * len(names), flags=flags)  # another column pitch
    chans = [A.open_channel(K['bitrate'], fs=K['fs']) for _ in names]
    msgs = [fi.messages(len(fi.stream(kind, n).pcm), '12000') for n in names]
    accs = [_new_acc(True) for _ in names]

    def feed(eng, chs, k):
        for n, ch, m in zip(names, chs, msgs):
            if k < len(m):
                eng.push(ch, fi.stream(kind, n).pcm[m[k][0]:m[k][1]])

    def take(eng, chs):
        for ch, acc in zip(chs, accs):
            acc['soft'] = np.concatenate([acc['soft'], eng.softbits(ch)])
            acc['blocks'] = np.concatenate([acc['blocks'], eng.blocks(ch)])
            acc['frames'] = np.concatenate([acc['frames'], eng.frames(ch)])
            acc['items'] += eng.items(ch)
            acc['edges'] = eng.channel_events(ch)[0]

    for k in range(at):
        feed(A, chans, k)
        A.run()
    feed(A, chans, at)  # pushed and not yet demodulated
    blob = A.export_channels(chans)
    take(A, chans)
    moved = B.import_channels(blob)
    assert len(moved) == len(chans)
    for k in range(at + 1, max(len(m) for m in msgs)):
        feed(B, moved, k)
        B.run()
    B.flush()
    take(B, moved)
    for n, acc, ref in zip(names, accs, refs):
        acc.pop('fragments')
        compare(acc, ref, '%s %s moved' % (kind, n))
    A.close()
    B.close()
