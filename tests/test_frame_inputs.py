"""What the streams of tests/frame_inputs.py reach, proved with the oracle
alone (no GPU): its link-layer trace (oracle_link_trace), frame records and
items.  tests/test_gpu_frame_inputs.py compares the engine with the oracle on
the same streams; a class that did not reach what its name promises would make
that comparison vacuous there, so it fails here."""
import numpy as np
import pytest

import aero_testlib as tl
import frame_inputs as fi

SYNC, WRAP, BLOCK, FRAME, TICK, RESET = tl.LK_SYNC, tl.LK_WRAP, tl.LK_BLOCK, tl.LK_FRAME, tl.LK_TICK, tl.LK_ISU_RESET
KINDS = tuple(fi.KINDS)
MSK = ('msk600', 'msk1200')


@pytest.fixture(scope='module', autouse=True)
def _libs(cpu_libs):
    import build
    build.build_oracletick()


def ref(kind, name, tick=False):
    return fi.reference(kind, name, '12000', tick)


def events(kind, name, tick=False):
    """the adversarial part's events with a fifth column: the channel bit"""
    s = fi.stream(kind, name)
    full = ref(kind, name, tick)['trace']
    lt = fi.adv_events(s, full)
    return s, np.column_stack([lt, lt[:, 1] + fi.lt_offset(s, full)])


def texts(out, key='items'):
    return [bytes.fromhex(l.split(' msg=')[1]) for l in out[key]]


def recovered(kind, name, tick=False):
    """the adversarial information fields the oracle hands back with every CRC good"""
    s = fi.stream(kind, name)
    per = fi.KINDS[kind]['info'] // 12
    good = [f for f, m in tl.frame_records(ref(kind, name, tick)['frames']) if m == (1 << per) - 1]
    adv = [f for f, _ in s.frames[s.lead:len(s.frames) - fi.KINDS[kind]['tail']]]
    return [f in good for f in adv]


def test_bits_entries_leave_the_old_ones_alone(cpu_libs):
    """the old entries are 'bits from Tx::next_frame*' over the same modulator:
    the Transmitter here restates Tx, so its bits through the new entry give
    the oracle the old entry's kind of stream; and silence follows the last bit"""
    bits = np.zeros(40, dtype=np.uint8)
    pcm = tl.synth_bits(bits, ebn0=99.0, lead_in=10, tail=3000)
    assert not pcm[:10].any() and pcm[10:400].any() and not pcm[-2000:].any()
    pcm = tl.synth_msk_bits(bits, ebn0=99.0, lead_in=10, tail=3000)
    assert not pcm[:10].any() and pcm[10:400].any() and not pcm[-2000:].any()


@pytest.mark.parametrize('kind', KINDS)
def test_lead_and_sizes(kind):
    L = fi.lead_frames(kind)
    assert 2 <= L < fi.LEAD_PROBE[kind]
    for name in fi.classes(kind):
        s = fi.stream(kind, name)
        assert s.lead == L and 0 < len(s.frames) - L - fi.KINDS[kind]['tail'] <= fi.MAX_ADV, name
        first = ref(kind, name)['trace']
        first = first[first[:, 0] == SYNC][0, 1] + fi.lt_offset(s, first)
        assert first + fi.KINDS[kind]['nbits'] <= s.adv_bit, '%s: a whole frame lies between the first sync and the part' % name
    for sched in fi.SCHEDULES:
        assert all(0 < b - a <= fi.CAP for a, b in fi.messages(400000, sched))


@pytest.mark.parametrize('kind', KINDS)
def test_plain_proves_the_builder(kind):
    assert all(recovered(kind, 'plain')), 'the transmitted information fields come back byte for byte, every CRC valid'
    s, ev = events(kind, 'plain')
    assert set(ev[:, 0]) == {SYNC, BLOCK, FRAME} and (ev[ev[:, 0] == SYNC][:, 2] == fi.KINDS[kind]['nbits'] - 1).all()
    assert ref(kind, 'plain')['items'] and ref(kind, 'plain')['edges'] == 1


@pytest.mark.parametrize('kind', KINDS)
def test_su_types(kind):
    assert all(recovered(kind, 'su_types'))
    out = ref(kind, 'su_types')
    firsts = {f[12 * k] for f, m in tl.frame_records(out['frames']) for k in range(len(f) // 12) if m >> k & 1}
    assert len(firsts) == 256 if kind == 'p10500' else {0x11, 0x21, 0x31, 0x32, 0x33, 0x34, 0x71, 0xC0, 0xFF} <= firsts
    t = b'|'.join(texts(out))
    for word in (b'Log on confirm', b'C_channel_assignment_distress', b'C_channel_assignment_flight_safety',
                 b'C_channel_assignment_other_safety', b'C_channel_assignment_non_safety', b'Call_announcement'):
        assert word in t, word


@pytest.mark.parametrize('kind', KINDS)
def test_crc_zero(kind):
    out = ref(kind, 'crc_zero')
    seen = {'zero_ok': 0, 'zero_crc_bad': 0, 'swap_bad': 0, 'crc_only': 0}
    sent = {f for f, _ in fi.stream(kind, 'crc_zero').frames[fi.stream(kind, 'crc_zero').lead:]}
    for f, m in tl.frame_records(out['frames']):
        if f not in sent:
            continue
        for k in range(len(f) // 12):
            su, ok = f[12 * k:12 * k + 12], m >> k & 1
            if su == fi.ZERO_SU:
                assert ok, 'the all-zero SU passes by the special case'
                seen['zero_ok'] += 1
            elif su[10:] == b'\0\0':
                assert not ok
                seen['zero_crc_bad'] += 1
            elif not any(su[:10]):
                assert not ok, 'zero data with a nonzero CRC fails'
                seen['crc_only'] += 1
            elif su[0] == 0x11 and fi.crc16(su[:10]) == su[10] << 8 | su[11]:
                assert not ok
                seen['swap_bad'] += 1
    assert all(v >= 2 for v in seen.values()), seen


@pytest.mark.parametrize('kind', KINDS)
def test_crc_mix(kind):
    s, ev = events(kind, 'crc_mix', tick=True)
    tk = ev[ev[:, 0] == TICK]
    assert -1 in tk[:, 3] and -2 in tk[:, 3], 'the timer takes 2 to -1 and 1 to -2'
    neg = np.nonzero(tk[:, 3] < 0)[0]
    assert any(k + 1 < len(tk) and tk[k + 1, 3] >= 0 for k in neg), 'and a later tick clamps'
    last = tk[neg[-1], 1]
    assert (ev[(ev[:, 0] == FRAME) & (ev[:, 1] > last)][:, 3] > 2).any(), 'the CRCs take it above 2 again'
    mk = [bin(m).count('1') for m in fi.masks(ref(kind, 'crc_mix', True))]
    assert len({m for m in mk if 0 < m < fi.KINDS[kind]['info'] // 12}) >= 2, 'mixed masks'
    assert ref(kind, 'crc_mix', True)['edges'] > ref(kind, 'crc_mix')['edges'] == 1, 'untimed, datacd never falls'


def test_uw_lost():
    kind = 'p10500'
    s, ev = events(kind, 'uw_lost', tick=True)
    ch = fi.model_datacd(ev[:, :4], True)
    assert [c[2] for c in ch[:2]] == ['tick', 'crc'], 'datacd falls at a tick and rises by CRCs alone'
    a, b = ch[0][0], ch[1][0]
    assert not (ev[a:b, 0] == SYNC).any(), 'no sync since the drop'
    ends = ev[:b][np.isin(ev[:b, 0], (SYNC, WRAP))]
    assert ends[-1, 0] == WRAP, 'the frame whose CRCs raise it is a flywheel frame'
    assert (ev[b:, 0] == SYNC).any(), 'then a good UW'
    assert ref(kind, 'uw_lost', True)['edges'] >= 3 and ref(kind, 'uw_lost')['edges'] == 1
    assert 1 <= fi.lost_lengths(kind)[0] and 1 <= fi.lost_lengths(kind)[1]


def test_uw_inverted():
    kind = 'p10500'
    s = fi.stream(kind, 'uw_inverted')
    out = ref(kind, 'uw_inverted')
    assert all(recovered(kind, 'uw_inverted')), 'valid frames after each polarity change'
    # the channel bits did change polarity arm by arm (the demodulator may follow such a change by
    # turning its phase, so the received arms are not compared): frames after it decode only if the
    # detectors' inversion flags follow
    true = fi.Transmitter(kind, 0)
    for info, edit in s.frames:
        true.frame(info, {k: v for k, v in (edit or {}).items() if k != 'pol'})
    diff = true.bits() ^ s.bits
    seen = set()
    for j in range(s.lead, len(s.frames) - 1):
        d = diff[s.starts[j]:s.starts[j + 1] - 64]
        assert d[0::2].min() == d[0::2].max() and d[1::2].min() == d[1::2].max()
        seen.add((int(d[0]), int(d[1])))
    assert seen == {(0, 0), (1, 1), (1, 0), (0, 1)}
    ev = events(kind, 'uw_inverted')[1]
    assert ref(kind, 'uw_inverted')['edges'] == 1 and not (ev[:, 0] == WRAP).any()


def test_uw_one_arm_and_skew():
    kind, nb = 'p10500', 5250
    s, ev = events(kind, 'uw_one_arm')
    assert (ev[:, 0] == WRAP).sum() == 3 and not (ev[:, 0] == RESET).any(), 'a UW on one arm alone never syncs'
    assert all(recovered(kind, 'uw_one_arm')), 'the flywheel frames decode'
    s, ev = events(kind, 'uw_skew')
    sy = ev[ev[:, 0] == SYNC]
    assert (sy[:, 2] == nb - 2).sum() == 1, 'the arms hit in the other order: a sync one bit early'
    k = np.nonzero((ev[:, 0] == SYNC) & (ev[:, 2] == nb - 2))[0][0]
    assert ev[k - 1, 0] == RESET
    # three bits apart the hits never pair: that frame ends by the flywheel
    j = s.lead + 4
    in_frame = ev[(ev[:, 4] > s.starts[j]) & (ev[:, 4] <= s.starts[j + 1] + 2)]
    assert (in_frame[:, 0] == WRAP).any() and not (in_frame[:, 0] == SYNC).any()


def test_uw_early_and_late():
    kind, nb = 'p10500', 5250
    lim = fi.shift_limits(kind)
    # the gate opens at cntr > 4992 - 68: the UW's 64 bits fit when the frame is at most 261 bits short
    # the gate opens behind cntr 4992 - 68: a frame up to 260 bits short has its whole UW inside (the limit
    # found lies a bit or two beyond: the detectors keep what they saw before the gate shut); the block
    # ends 64 bits before the frame; behind the frame's end the gate is open for cntr <= 0
    assert 260 <= lim['early'] <= 264 and lim['block'] == 64 and lim['late'] == 2, lim
    s, ev = events(kind, 'uw_early')
    sy = ev[ev[:, 0] == SYNC][:, 2]
    for d in (lim['block'], lim['block'] + 1, lim['early']):
        assert (sy == nb - 1 - d).sum() == 1, d
    assert not (sy == nb - 2 - lim['early']).any(), 'one bit outside the window'
    for d, done in ((lim['block'], True), (lim['block'] + 1, False)):
        k = np.nonzero((ev[:, 0] == SYNC) & (ev[:, 2] == nb - 1 - d))[0][0]
        frame = ev[:k][ev[:k, 1] > ev[k, 1] - (nb - d)]
        assert (frame[:, 0] == FRAME).any() == done, 'the block %s before the early UW' % ('ends' if done else 'is lost')
        assert ev[k - 1, 0] == RESET
    s, ev = events(kind, 'uw_late')
    sy = ev[ev[:, 0] == SYNC][:, 2]
    assert (sy == lim['late'] - 1).sum() == 1 and not (sy == lim['late']).any()
    # untimed, the frame that is one bit too long loses the channel for good: the gate stays shut
    assert (ev[:, 0] == WRAP).sum() >= 5 and not all(recovered(kind, 'uw_late'))


def test_uw_in_data():
    kind, nb = 'p10500', 5250
    s, ev = events(kind, 'uw_in_data')
    assert (ev[ev[:, 0] == SYNC][:, 2] == nb - 1).all(), 'with datacd set a UW in the data area is ignored'
    s, ev = events(kind, 'uw_in_data_drop', tick=True)
    ch = fi.model_datacd(ev[:, :4], True)
    assert ch[0][2] == 'tick'
    mid = ev[(ev[:, 0] == SYNC) & (ev[:, 2] > 194) & (ev[:, 2] < 194 + 4992 - 68)]
    assert len(mid) >= 1 and mid[0, 1] > ev[ch[0][0], 1], 'after the drop it resyncs mid-frame'
    s, ev = events(kind, 'uw_in_data_drop')
    assert not ((ev[:, 0] == SYNC) & (ev[:, 2] < nb - 1)).any(), 'untimed it never does'


def test_header():
    seen = set()
    for name in ('header_lo', 'header_hi'):
        out = ref('p10500', name)
        t = texts(out)
        with_p = [x for x in t if b'format ID error\n' in x]
        without = [x for x in t if b'C_channel_assignment' in x and b'format ID error\n' not in x]
        assert with_p and without, 'items with and without the prefix'
        assert all(x.split(b'\r\n')[1].startswith(b'format ID error\n0 ') for x in with_p), 'SU 0 alone carries it'
        assert any(x.split(b'\r\n')[1].startswith(b'1 ') for x in without)
        seen |= {e['format'] for _, e in fi.stream('p10500', name).frames if e}
    assert seen == set(range(16))


@pytest.mark.parametrize('kind', KINDS)
def test_isu_paths(kind):
    t = b'|'.join(texts(ref(kind, 'isu_paths')))
    for word, there in ((b'SECOND', True), (b'FIRST ISU', False), (b'AFTER 10 ISUS', True), (b'AFTER 11 ISUS', False),
                        (b'AES ZERO', False), (b'NOOCT NINE', False)):
        assert (word in t) == there, word
    assert (b'OVERLONG..' + bytes(6)).hex().upper().encode() in t, 'the SSU read past its end gives zeros'
    if kind == 'p10500':
        assert max(len(x) for x in texts(ref(kind, 'isu_paths'))) >= 2 + 63 * 8 - 22, 'the 63-SSU message'
    assert all(recovered(kind, 'isu_paths'))


def test_isu_split_and_acars_paths():
    kind = 'p10500'
    t = texts(ref(kind, 'isu_split'))
    assert sum(b'SPLIT OVER FRAMES' in x for x in t) == 1, 'clean: once; across a reset and across eleven ISUs: not'
    s, ev = events(kind, 'isu_split')
    assert (ev[:, 0] == RESET).sum() == 1
    out = ref(kind, 'acars_paths')
    t = b'|'.join(texts(out))
    for word, there in ((b'REG PARITY', False), (b'TEXT PARITY', False), (b'DEL<DEL>X', True),
                        (b'PART A PART B PART C ', True), (b'WRAP Y WRAP Z WRAP A ', True), (b'TAK ONE TAK TWO', False),
                        (b'TAK TWO', True)):
        assert (word in t) == there, word
    assert sum(' nonacars=1' in l for l in out['items']) >= 2
    assert len(out['fragments']) >= sum(' nonacars=0' in l for l in out['items']) + 4, 'two chains of three blocks'
    t = b'|'.join(texts(ref(kind, 'acars_expiry')))
    for word, there in ((b'EXPIRES TOO LATE', False), (b'TOO LATE', True), (b'KEPT IN TIME', True)):
        assert (word in t) == there, word


def test_noisy():
    kind = 'p10500'
    m = fi.masks(ref(kind, 'noisy'))[-6:]
    share = sum(bin(x).count('1') for x in m) / (26.0 * 6)
    assert 0.25 <= share <= 0.75, share


@pytest.mark.parametrize('kind', MSK)
def test_msk_uw_classes(kind):
    nb = 1200
    B = 64 * fi.KINDS[kind]['N']
    s, ev = events(kind, 'uw_missing')
    assert (ev[:, 0] == WRAP).sum() == 3 and all(recovered(kind, 'uw_missing')), 'three flywheel frames that decode'
    for name, at in (('uw_in_data1', {16 + B + 39, 16 + B - 1}), ('uw_in_data2', {16 + 2 * B - 1})):
        s, ev = events(kind, name)
        mid = ev[(ev[:, 0] == SYNC) & (ev[:, 2] < nb - 1)]
        assert at <= set(mid[:, 2]) and (ev[:, 0] == RESET).sum() >= 2, name
    # the infofield is cleared with blocks of the broken frame in it, and a frame ends on the sync bit itself
    if kind == 'msk1200':
        k = np.nonzero((ev[:, 0] == SYNC) & (ev[:, 2] == 16 + 2 * B - 1))[0][0]
        assert ev[k - 2, 0] == FRAME and ev[k - 2, 1] == ev[k, 1]
    s, ev = events(kind, 'uw_train', tick=True)
    sy = ev[ev[:, 0] == SYNC][:, 1]
    assert max(int(((sy >= x) & (sy < x + 216)).sum()) for x in sy) >= 4, 'at least 4 syncs within one 216-bit hop'
    assert (np.diff(sy) == 32).sum() >= 20
    s, ev = events(kind, 'uw_early')
    assert ((ev[:, 0] == SYNC) & (ev[:, 2] == nb - 2)).sum() == 2
    s, ev = events(kind, 'uw_late')
    assert ((ev[:, 0] == SYNC) & (ev[:, 2] == 0)).sum() == 2 and (ev[:, 0] == WRAP).sum() == 2


@pytest.mark.parametrize('kind', KINDS)
def test_where_the_tick_changes_the_outcome(kind):
    for name in fi.classes(kind):
        a, b = ref(kind, name), ref(kind, name, True)
        differs = a['edges'] != b['edges'] or not np.array_equal(a['frames'], b['frames']) or a['items'] != b['items']
        if name in fi.TICK_CLASSES and not (kind != 'p10500' and name == 'uw_train'):
            assert differs, name
    # continuous MSK framing never reads datacd: the timer moves the DataCarrierDetect changes alone
    if kind != 'p10500':
        for name in fi.classes(kind):
            a, b = ref(kind, name), ref(kind, name, True)
            assert np.array_equal(a['frames'], b['frames']) and a['items'] == b['items'], name


def test_msk1200_lock_at_24k():
    """why the 1200-bps streams are made at 12 kHz: at 24 kHz the reference's
    demodulator drops a clean 600-baud carrier within 20 frames"""
    pcm = tl.synth_msk(seconds=40.0, bitrate=1200, baud=600, ebn0=20.0, carrier=1800.0)
    o = tl.Oracle(bitrate=1200)
    o.push_chunked(pcm, 12000)
    m = [x for _, x in tl.frame_records(o.frames())]
    assert 0x3f in m and m[-8:].count(0x3f) < 8 and m.index(0x3f) + 10 < len(m)
    assert 0 in m[m.index(0x3f):], 'frames fail after the first good one'


def test_sensitivity_of_the_comparison():
    """an oracle reference altered in one mask bit of crc_zero, one countdown
    step of crc_mix or the clear decision of uw_in_data fails the GPU test's
    comparison (tests/test_gpu_frame_inputs.py compare) at that class"""
    import test_gpu_frame_inputs as g
    for kind, name, tick in (('p10500', 'crc_zero', False), ('msk600', 'crc_zero', False), ('p10500', 'crc_mix', True),
                             ('msk600', 'crc_mix', True), ('msk600', 'uw_in_data1', False)):
        good = ref(kind, name, tick)
        g.compare(good, good, name)
        for bad in g.altered(kind, name, good):
            with pytest.raises(AssertionError):
                g.compare(bad, good, name)
