"""Adversarial frame content for the stage between the demodulator's soft
bits and the ACARS items: the framing kernels (aerol.hip frame_kernel,
frame_msk_kernel), the Viterbi's post step (delay line, scrambler, CRCs), the
host assembly of engine.hip process_slot and PChannelHost (acars_host.cpp).

A numpy transmitter builds channel bits from information fields (scrambler,
K = 7 encoder carried across frames, 64-row interleaver, header, UW) and edits
the finished bits per frame; tools/aero_synth.cpp modulates them
(aero_synth_p10500_bits / aero_synth_msk_bits).  An SU grammar on top makes
the information fields.  tests/test_frame_inputs.py proves with the oracle
alone (oracle_link_trace, frame records, items) what every class reaches;
tests/test_gpu_frame_inputs.py compares the engine with the oracle on them;
tests/test_host_su_fuzz.py feeds the curated information fields to
PChannelHost past the modem.

Every stream is a lead of plain frames (lead_frames: searched with the
oracle), at most 10 adversarial frames and TAIL plain ones that carry the
adversarial content through the delay line.  Everything is seeded; what
depends on the decoder (the lead, the shift limits of uw_early / uw_late, the
Eb/N0 of noisy, the CRC patterns of crc_mix, the drop lengths of uw_lost) is
searched with the oracle, and a search that finds nothing raises
AssertionError."""
import ctypes
import functools

import numpy as np

import aero_testlib as tl
import cont_dcd_lib as cd

SEED = 0xF4A3
UW = 0xE15AE893
MAX_ADV = 10
CAP = 32768  # the largest message the PCM ring admits (PCM_CAP / 2)

KINDS = {
    'p10500': dict(bitrate=10500, fs=48000, baud=10500, info=312, nbits=5250, N=78, hdr=194, data=4992, tail=3,
                   carrier=12037.5, ebn0=14.0),
    'msk600': dict(bitrate=600, fs=12000, baud=600, info=72, nbits=1200, N=6, hdr=16, data=1152, tail=2,
                   carrier=1800.0, ebn0=14.0),
    # 1200-bps framing at 600 baud, the only modulation rate `-b 1200` demodulates.  At 12 kHz: at the
    # 24 kHz aero-decode feeds `-b 1200` the reference's demodulator keeps its lock for about seven
    # 2-s frames at a time (test_frame_inputs.py::test_msk1200_lock_at_24k), less than a lead and ten frames
    'msk1200': dict(bitrate=1200, fs=12000, baud=600, info=72, nbits=1200, N=9, hdr=16, data=1152, tail=2,
                    carrier=1800.0, ebn0=14.0),
}
SCHEDULES = ('3000', '12000', 'ragged')


def spf(kind):
    """samples per frame"""
    k = KINDS[kind]
    return k['nbits'] * k['fs'] // k['baud']


def messages(n, schedule):
    """[start, stop) of the messages of an n-sample stream, one per run()"""
    sizes = {'3000': (3000,), '12000': (12000,), 'ragged': tuple(min(s, CAP) for s in tl.RAGGED)}[schedule]
    out, p, k = [], 0, 0
    while p < n:
        out.append((p, min(n, p + sizes[k % len(sizes)])))
        p = out[-1][1]
        k += 1
    return out


# ------------------------------------------------------------------ SU grammar
def crc16(b):
    return int(tl.Oracle.lib().oracle_crc16_bytes(bytes(b), len(b)))


def odd(c):
    c &= 0x7F
    return c if bin(c).count('1') & 1 else c | 0x80


def make_su(ten, crc='ok'):
    """12 bytes: ten + CRC-16/X-25 little endian; crc: ok / bad (one bit of it
    wrong) / zero (both bytes 0) / swap (big endian)"""
    ten = bytes(ten)
    assert len(ten) == 10
    c = crc16(ten)
    lo, hi = c & 0xFF, c >> 8
    if crc == 'bad':
        lo ^= 0x10
    elif crc == 'zero':
        assert c != 0 or not any(ten)
        lo = hi = 0
    elif crc == 'swap':
        assert lo != hi, 'a palindromic CRC cannot be swapped'
        lo, hi = hi, lo
    else:
        assert crc == 'ok'
    return ten + bytes([lo, hi])


ZERO_SU = bytes(12)  # what the CRC check's special case accepts (decode/aerol.cpp:1540-1544)


def acars_ud(reg='.N12345', label='H1', bi='A', text='', more=False, mode='2', tak=0x15, stx=True, bad=(), bcs=(0x41, 0x42)):
    """ACARS user data as ParserISU reads it (decode/aerol.cpp:333-489): FF FF
    SOH mode reg(7) TAK label(2) BI STX text ETX/ETB BCS BCS DEL.  stx=False:
    no text (ETX at byte 15).  bad: byte positions whose parity bit is flipped."""
    ud = [0xFF, 0xFF, odd(0x01), odd(ord(mode))] + [odd(ord(c)) for c in (reg + '.......')[:7]]
    ud += [odd(tak), odd(ord(label[0])), odd(ord(label[1])), odd(ord(bi) if isinstance(bi, str) else bi)]
    if stx:
        ud += [0x02] + [odd(ord(c)) if isinstance(c, str) else c for c in text]
    ud += [0x97 if more else 0x83, bcs[0], bcs[1], 0x7F]
    for k in bad:
        ud[k] ^= 0x80
    return bytes(ud)


def isu_chain(aes, ges, qno, ref, ud, rng=None, nooct=None, seqno=None):
    """[0x71 ISU, SSU m-1 .. SSU 0] carrying ud (ISUData::update, decode/aerol.cpp:158-227)"""
    rest = len(ud) - 2
    m = max(1, (rest + 7) // 8)
    r = rest - 8 * (m - 1)
    key = ((qno & 15) << 4) | (ref & 15)
    isu = [0x71, (aes >> 16) & 255, (aes >> 8) & 255, aes & 255, ges, key, (m if seqno is None else seqno) & 0x3F,
           ((r if nooct is None else nooct) & 15) << 4, ud[0], ud[1]]
    out, p = [make_su(isu)], 2
    for s in range(m - 1, -1, -1):
        nb = r if s == 0 else 8
        pad = [int(rng.integers(256)) if rng is not None else 0 for _ in range(8 - nb)]
        out.append(make_su([0xC0 | s, key] + list(ud[p:p + nb]) + pad))
        p += nb
    return out


class Grammar:
    """seeded plain traffic: fill SUs, log-on confirms, C channel assignments, valid ACARS"""

    def __init__(self, *seed):
        self.rng = np.random.default_rng([SEED] + [int(s) for s in seed])
        self.aes = [0x400000 + int(self.rng.integers(0x3FFFFF)) for _ in range(8)]
        self.ref = 0
        self.queue = []

    def rand(self, n):
        return [int(v) for v in self.rng.integers(0, 256, n)]

    def text(self, n):
        alpha = 'ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 /.-,:'
        return ''.join(alpha[int(i)] for i in self.rng.integers(0, len(alpha), n))

    def fill(self):
        return make_su([0x01] + self.rand(9))

    def typed(self, first, aes=None):
        aes = self.aes[int(self.rng.integers(8))] if aes is None else aes
        return make_su([first, aes >> 16, (aes >> 8) & 255, aes & 255, 0x80 + int(self.rng.integers(8))] + self.rand(5))

    def acars(self, text=None, **kw):
        aes = kw.pop('aes', self.aes[int(self.rng.integers(8))])
        ges = kw.pop('ges', 0x80 + int(self.rng.integers(8)))
        qno = kw.pop('qno', int(self.rng.integers(16)))
        self.ref += 1
        ref = kw.pop('ref', self.ref)
        kw.setdefault('reg', '.N%05u' % (aes % 100000))
        kw.setdefault('label', ('H1', 'SA', '_d', 'Q0', 'B6', '10', '5Z', 'AA')[int(self.rng.integers(8))])
        ud = acars_ud(text=self.text(int(self.rng.integers(0, 40))) if text is None else text, **kw)
        return isu_chain(aes, ges, qno, ref, ud, self.rng)

    def refill(self):
        u = self.rng.random()
        if u < 0.5:
            self.queue += self.acars()
        elif u < 0.6:
            self.queue.append(self.typed(0x11))
        elif u < 0.7:
            self.queue.append(self.typed(0x34))
        else:
            self.queue.append(self.fill())

    def take(self, n):
        while len(self.queue) < n:
            self.refill()
        out, self.queue = self.queue[:n], self.queue[n:]
        return out

    def frames(self, kind, n):
        """n plain information fields"""
        per = KINDS[kind]['info'] // 12
        return [b''.join(self.take(per)) for _ in range(n)]

    def pack(self, kind, sus):
        """sus as whole information fields, the last one filled up with fill SUs"""
        per = KINDS[kind]['info'] // 12
        sus = list(sus)
        while len(sus) % per:
            sus.append(self.fill())
        return [b''.join(sus[i:i + per]) for i in range(0, len(sus), per)]


# ------------------------------------------------------------------ transmitter
@functools.lru_cache(maxsize=None)
def _scr():
    s = np.zeros(5000, dtype=np.int32)
    tl.Oracle.lib().oracle_scrambler_bits(s.ctypes.data_as(ctypes.c_void_p), 5000)
    return s.astype(np.uint8)


PERM = np.array([(27 * i) % 64 for i in range(64)])


def uw_bits(word):
    return np.array([(word >> (31 - j)) & 1 for j in range(32)], dtype=np.uint8)


class Transmitter:
    """information fields -> channel bits, frame by frame (what
    tools/aero_synth.cpp Tx::next_frame / next_frame_msk transmit, restated so
    that every part can be edited).  edit (dict, all optional):
      header  the 16 header bits' value (default 0x1000 | frame counters)
      format  the format id alone (the header's top nibble)
      uw      10500: (Q word, I word); MSK: word; None in their place: 32 seeded random bits
      skew_i  10500: the I arm's UW moved by this many arm symbols (+ later, - earlier)
      write   [(position, bits)] written over the finished frame
      remove  (position, n): n bits taken out;  insert (position, n): n seeded bits put in
      pol     10500: (Q, I) arm polarity (True: complemented) from this frame's UW on"""

    def __init__(self, kind, *seed):
        self.kind, self.k = kind, KINDS[kind]
        self.hist = np.zeros(6, dtype=np.uint8)  # the encoder's last six input bits
        self.frame_no = 0
        self.rng = np.random.default_rng([SEED, 7] + [int(s) for s in seed])
        self.pol = (False, False)
        self.out = []     # bits of the frames so far
        self.total = 0    # their count
        self.starts = []  # first bit of every frame

    def _encode(self, info):
        k = self.k
        n = 8 * k['info']
        assert len(info) == k['info']
        bits = np.unpackbits(np.frombuffer(info, dtype=np.uint8), bitorder='little') ^ _scr()[:n]
        b = np.concatenate([self.hist, bits])
        t = np.arange(6, 6 + n)
        c0 = b[t] ^ b[t - 2] ^ b[t - 3] ^ b[t - 5] ^ b[t - 6]  # 109
        c1 = b[t] ^ b[t - 1] ^ b[t - 2] ^ b[t - 3] ^ b[t - 6]  # 79
        self.hist = b[-6:].copy()
        coded = np.empty(2 * n, dtype=np.uint8)
        coded[0::2], coded[1::2] = c0, c1
        N = k['N']
        B = 64 * N
        data = np.empty(2 * n, dtype=np.uint8)
        for b0 in range(0, 2 * n, B):  # block[perm[i] * N + j] = coded[j * 64 + i]
            blk = coded[b0:b0 + B].reshape(N, 64)  # [j, i]
            dst = np.empty((64, N), dtype=np.uint8)
            dst[PERM, :] = blk.T
            data[b0:b0 + B] = dst.reshape(-1)
        return data

    def frame(self, info, edit=None):
        e, k = dict(edit or {}), self.k
        chan = np.zeros(k['nbits'], dtype=np.uint8)
        fc = self.frame_no & 15
        hdr = 0x1000 | (((self.frame_no >> 4) & 15) << 8) | (fc << 4) | fc
        if 'format' in e:
            hdr = (hdr & 0x0FFF) | ((e.pop('format') & 15) << 12)
        hdr = e.pop('header', hdr)
        chan[:16] = [(hdr >> (15 - b)) & 1 for b in range(16)]
        if k['hdr'] > 16:
            chan[16:k['hdr']] = self.rng.integers(0, 2, k['hdr'] - 16)
        chan[k['hdr']:k['hdr'] + k['data']] = self._encode(info)
        u0 = k['hdr'] + k['data']
        rnd = lambda: self.rng.integers(0, 2, 32).astype(np.uint8)
        uw = e.pop('uw', (UW, UW) if self.kind == 'p10500' else UW)
        if self.kind == 'p10500':
            q, i = [rnd() if w is None else uw_bits(w) for w in uw]
            chan[u0::2], chan[u0 + 1::2] = q, i
            sk = e.pop('skew_i', 0)
            if sk:
                chan[u0 + 1::2] = self.rng.integers(0, 2, 32)
                at = u0 + 1 + 2 * sk
                assert sk < 0, 'a later I arm runs into the next frame: use a negative skew on the next frame'
                chan[at:at + 64:2] = i
        else:
            chan[u0:] = rnd() if uw is None else uw_bits(uw)
        for pos, bits in e.pop('write', ()):
            chan[pos:pos + len(bits)] = bits
        if 'remove' in e:
            pos, n = e.pop('remove')
            chan = np.delete(chan, np.arange(pos, pos + n))
        if 'insert' in e:
            pos, n = e.pop('insert')
            chan = np.insert(chan, pos, self.rng.integers(0, 2, n).astype(np.uint8))
        pol = e.pop('pol', None)
        assert not e, 'unknown edit %r' % sorted(e)
        idx = self.total + np.arange(len(chan))
        for arm, was, now in ((0, self.pol[0], (pol or self.pol)[0]), (1, self.pol[1], (pol or self.pol)[1])):
            on = np.where(np.arange(len(chan)) >= len(chan) - 64, now, was)
            chan = chan ^ ((idx % 2 == arm) & on).astype(np.uint8)
        if pol:
            self.pol = tuple(pol)
        self.frame_no += 1
        self.starts.append(self.total)
        self.total += len(chan)
        self.out.append(chan)
        return chan

    def bits(self):
        return np.concatenate(self.out)


def modulate(kind, bits, ebn0=None):
    k = KINDS[kind]
    e = k['ebn0'] if ebn0 is None else ebn0
    if kind == 'p10500':
        return tl.synth_bits(bits, seed=SEED, carrier=k['carrier'], ebn0=e)
    # a third of a second behind the last bit: the demodulator's delays and its groups of 12 deliver the last UW
    return tl.synth_msk_bits(bits, bitrate=k['bitrate'], baud=k['baud'], seed=SEED, carrier=k['carrier'], ebn0=e,
                             fs=k['fs'], tail=k['fs'] // 3)


LEAD_IN = {'p10500': 1000, 'msk600': 500, 'msk1200': 500}
LEAD_PROBE = {'p10500': 30, 'msk600': 24, 'msk1200': 24}  # plain frames the lead is searched in


def _lead_infos(kind, n):
    return Grammar(1, KINDS[kind]['bitrate']).frames(kind, n)


class SkipTick(cd.ContTickOracle):
    """the hooked oracle with the timer on the sample clock (for 10500 bps what
    ORACLE_DCD_TICK does inside), its k-th tick left out: a reference that is
    wrong in one countdown step"""

    def __init__(self, bitrate, fs, skip):
        super().__init__(bitrate, fs)
        self.skip, self.fired = skip, 0

    def push(self, pcm, fs=None):
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        p = 0
        for q in self.clock.cuts(len(pcm)):
            tl.Oracle.push(self, pcm[p:q], self.clock.fs)
            if self.fired != self.skip:
                self.L.oracle_x_dcd_tick(self.h)
            self.fired += 1
            p = q
        if p < len(pcm):
            tl.Oracle.push(self, pcm[p:], self.clock.fs)


def make_oracle(kind, tick, skip_tick=None):
    k = KINDS[kind]
    if skip_tick is not None:
        return SkipTick(k['bitrate'], k['fs'], skip_tick)
    if kind == 'p10500':
        return tl.Oracle(dcd_tick=tick)
    return cd.ContTickOracle(k['bitrate'], k['fs'], tick=tick)


@functools.lru_cache(maxsize=None)
def lead_frames(kind):
    """The shortest lead of plain frames after which the oracle's first UW sync
    precedes the adversarial part under every schedule, plus one frame, plus
    the frames the delay line holds (the kind's tail): the first information
    fields after the sync come out of a delay line filled before it and fail
    their CRCs, and the adversarial part is to start from a countdown of 12."""
    tx = Transmitter(kind, 0)
    for info in _lead_infos(kind, LEAD_PROBE[kind]):
        tx.frame(info)
    pcm = modulate(kind, tx.bits())
    worst = 0
    for sched in SCHEDULES:
        o = make_oracle(kind, False)
        fed = None
        for a, b in messages(len(pcm), sched):
            o.push(pcm[a:b])
            lt = o.link_trace()
            if len(lt) and (lt[:, 0] == tl.LK_SYNC).any():
                fed = b
                break
        assert fed is not None, '%s: the oracle never syncs on the plain stream (%s)' % (kind, sched)
        worst = max(worst, -(-(fed - LEAD_IN[kind]) // spf(kind)))
    assert worst + 1 + KINDS[kind]['tail'] < LEAD_PROBE[kind]
    return worst + 1 + KINDS[kind]['tail']


class Stream:
    """one class's stream: pcm, the transmitted information fields and edits,
    where the adversarial part starts"""

    def __init__(self, kind, name, adv, ebn0=None, gram=None, adv_ebn0=None):
        assert 0 < len(adv) <= MAX_ADV, '%s/%s: %d adversarial frames' % (kind, name, len(adv))
        L = lead_frames(kind)
        gram = gram or Grammar(3, KINDS[kind]['bitrate'], sum(name.encode()))
        tx = Transmitter(kind, 0)
        self.frames = [(i, None) for i in _lead_infos(kind, LEAD_PROBE[kind])[:L]] + list(adv) + \
                      [(i, None) for i in gram.frames(kind, KINDS[kind]['tail'])]
        for info, edit in self.frames:
            tx.frame(info, edit)
        self.kind, self.name, self.lead = kind, name, L
        self.starts, self.bits = tx.starts, tx.bits()
        self.adv_bit = tx.starts[L]
        self.pcm = modulate(kind, self.bits, ebn0)
        per = KINDS[kind]['fs'] / float(KINDS[kind]['baud'])
        self.adv_sample = LEAD_IN[kind] + int(self.adv_bit * per)
        if adv_ebn0 is not None:
            # noise added over the adversarial frames alone, up to a nominal Eb/N0 (unit pulse energy):
            # the lead locks at the kind's own Eb/N0 and the tail carries the content out
            A = 0.25 * 32768
            var = lambda e: A * A * KINDS[kind]['fs'] / (2.0 * KINDS[kind]['bitrate'] * 10 ** (e / 10.0))
            sigma = np.sqrt(var(adv_ebn0) - var(KINDS[kind]['ebn0'] if ebn0 is None else ebn0))
            end = LEAD_IN[kind] + int(tx.starts[L + len(adv)] * per)
            noise = np.random.default_rng([SEED, 9]).normal(0, sigma, end - self.adv_sample)
            x = self.pcm.astype(np.float64)
            x[self.adv_sample:end] += noise
            self.pcm = np.clip(np.round(x), -32768, 32767).astype(np.int16)
        self.pcm.setflags(write=False)


def outputs(o):
    return dict(soft=o.softbits(), blocks=o.blocks(), frames=o.frames(), items=o.item_lines('A'),
                fragments=o.item_lines('F'), edges=o.events()[0], trace=o.link_trace())


def run_oracle(kind, pcm, schedule='12000', tick=False, per_run=False, skip_tick=None):
    """the oracle over pcm in the schedule's messages: its outputs; per_run:
    and after every message (soft bits, frame bytes, items, edges) so far"""
    o = make_oracle(kind, tick, skip_tick)
    steps = []
    for a, b in messages(len(pcm), schedule):
        o.push(pcm[a:b])
        if per_run:
            L = o.L
            steps.append((L.oracle_softbits(o.h, None, 0), L.oracle_frames(o.h, None, 0), o.events()[0]))
    out = outputs(o)
    if per_run:
        out['steps'] = steps
    return out


# ------------------------------------------------------------------ trace reading
@functools.lru_cache(maxsize=None)
def _lead_lock(kind):
    """(soft bits the oracle has taken at its first sync, channel bits sent
    before its first soft bit) on the kind's lead; soft bit n is channel bit
    n + offset while the demodulator stays locked.  From the plain stream: its
    last sync ends its last frame."""
    s = stream(kind, 'plain')
    out = run_oracle(kind, s.pcm)
    lt, nb = out['trace'], KINDS[kind]['nbits']
    sy = lt[lt[:, 0] == tl.LK_SYNC]
    assert len(sy) and sy[-1, 2] == nb - 1, 'no sync at a frame\'s end'
    # the last sync ends one of the last frames; which one: the soft bits run on to the stream's end
    # (less the demodulator's delay, plus what the noise behind the last bit gives: a fraction of a frame)
    est = len(s.bits) - len(out['soft'])
    off = min((len(s.bits) - j * nb - int(sy[-1, 1]) for j in range(4)), key=lambda o: abs(o - est))
    assert abs(off - est) < nb // 4, 'the last sync cannot be placed'
    first = int(sy[0, 1]) + off
    assert 0 < first <= s.adv_bit and first % KINDS[kind]['nbits'] == 0, 'the first sync does not end a lead frame'
    return int(sy[0, 1]), off


@functools.lru_cache(maxsize=None)
def drop_frames(kind):
    """uw_in_data_drop: the fewest UW-less frames with failing SUs after which
    the ticked oracle has dropped datacd before the next frame's data area
    (its SUs come out of the delay line frames later): a doubled UW written
    there then gives a sync in mid-frame"""
    K = KINDS[kind]
    two = np.repeat(np.concatenate([uw_bits(UW), uw_bits(UW)]), 2)
    for n in range(1, MAX_ADV - 2):
        g = Grammar(5, n)
        adv = _drop(kind, g, n, 0) + [(g.frames(kind, 1)[0], dict(write=[(K['hdr'] + 2400, two)]))] + \
              [(f, None) for f in g.frames(kind, 2)]
        s = Stream(kind, 'probe', adv, gram=g)
        lt = adv_events(s, run_oracle(kind, s.pcm, tick=True)['trace'])
        if ((lt[:, 0] == tl.LK_SYNC) & (lt[:, 2] > K['hdr']) & (lt[:, 2] < K['hdr'] + K['data'] - 68)).any():
            return n
    raise AssertionError('%s: datacd never drops before a data area' % kind)


def lt_offset(s, lt):
    """the lead is the same in every stream of a kind, and so is its lock"""
    first, off = _lead_lock(s.kind)
    assert int(lt[lt[:, 0] == tl.LK_SYNC][0, 1]) == first, 'the lead locked elsewhere'
    return off


def adv_events(s, lt):
    """the trace's events of the adversarial part and the tail"""
    return lt[lt[:, 1] + lt_offset(s, lt) > s.adv_bit]


def model_datacd(lt, dcd=False):
    """datacd along the trace from `dcd`: set by a sync, cleared by a tick that
    leaves the countdown at 0, set by a frame whose CRCs leave it above 2.
    Returns [(event index, new value, by)]."""
    out = []
    for i, (kind, _, _, cdn) in enumerate(lt):
        if kind == tl.LK_SYNC and not dcd:
            dcd = True
            out.append((i, True, 'sync'))
        elif kind == tl.LK_TICK and dcd and cdn == 0:
            dcd = False
            out.append((i, False, 'tick'))
        elif kind == tl.LK_FRAME and not dcd and cdn > 2:
            dcd = True
            out.append((i, True, 'crc'))
    return out


def masks(out):
    return [m for _, m in tl.frame_records(out['frames'])]


# ------------------------------------------------------------------ classes
def _su_types(kind, g):
    per = KINDS[kind]['info'] // 12
    if kind == 'p10500':
        firsts = list(range(256))
    else:  # 60 SUs: every dispatch branch, the SSU range's ends, seeded others
        special = [0x11, 0x21, 0x31, 0x32, 0x33, 0x34, 0x71, 0xC0, 0xC1, 0xFF, 0x00, 0x01, 0x30, 0x35, 0x70, 0x72, 0xBF]
        rest = [b for b in g.rng.permutation(256) if b not in special]
        firsts = special + [int(b) for b in rest[:MAX_ADV * per - len(special)]]
    return [(f, None) for f in g.pack(kind, [g.typed(b) for b in firsts])]


def _crc_zero(kind, g):
    per = KINDS[kind]['info'] // 12
    sus = []
    for k in range(3 * per):
        ten = [0x11] + g.rand(9)
        while crc16(ten) >> 8 == crc16(ten) & 255:
            ten = [0x11] + g.rand(9)
        sus.append([ZERO_SU, make_su([0] * 9 + [1 + k % 255], 'zero'), make_su(g.rand(10), 'zero'),
                    make_su(ten, 'swap'), g.typed(0x11), bytes(10) + bytes([0, 1]),
                    bytes(10) + bytes([1, 0])][k % 7])
    return [(f, None) for f in g.pack(kind, sus)]


def _masked(kind, g, ok):
    """one information field whose SU k has a good CRC where ok[k]"""
    return b''.join(s if good else s[:10] + bytes([s[10] ^ 0x10, s[11]]) for s, good in zip(g.take(len(ok)), ok))


def _header(kind, g, ids):
    out = []
    for n, fid in enumerate(ids):
        per = KINDS[kind]['info'] // 12
        sus = g.take(per)
        sus[n % 2] = g.typed(0x31 + n % 4)  # a C channel assignment in position 0 / 1
        out.append((b''.join(sus), dict(format=fid)))
    return out


def isu_path_sus(g, long=True):
    """the ISU / SSU cases of PChannelHost::isu_update (ISUData::update)"""
    aes = g.aes
    sus = []
    sus.append(make_su([0xC3, 0x5A] + g.rand(8)))  # an SSU without its ISU
    sus += isu_chain(aes[0], 0x81, 1, 1, acars_ud(text='NOOCT NINE'), g.rng, nooct=9)  # never matches
    sus += isu_chain(aes[0], 0x81, 1, 2, b'\x12\x34', g.rng, seqno=0)[:1]  # SEQNO 0: waits for SSU 255
    sus += isu_chain(aes[1], 0x82, 2, 3, bytes(g.rand(7)), g.rng)  # SEQNO 1, non-ACARS
    if long:
        sus += isu_chain(aes[2], 0x83, 3, 4, acars_ud(text=g.text(2 + 63 * 8 - 22)), g.rng)  # SEQNO 63
    # replacement: the second ISU with the same (aes, ges, qno, ref) takes the first's place
    a = isu_chain(aes[3], 0x84, 4, 5, acars_ud(text='FIRST ISU, REPLACED'), g.rng)
    b = isu_chain(aes[3], 0x84, 4, 5, acars_ud(text='SECOND'), g.rng)
    sus += a[:2] + b + a[2:]
    # expiry: after ten further 0x71 the ISU still waits, after eleven it is gone
    for n in (10, 11):
        x = isu_chain(aes[4], 0x85, 5, 6 + n, acars_ud(text='AFTER %d ISUS' % n), g.rng)
        sus += x[:1]
        for j in range(n):
            # (an SSU is matched with the AES and GES of the last 0x71, so the others are this aircraft's)
            sus += isu_chain(aes[4], 0x85, 6, j, b'\x00\x00', g.rng, seqno=0)[:1]
        sus += x[1:]
    # an ISU that says 14 octets in its last SSU never matches by itself, but it is completed once a
    # later 0x71 of the same AES / GES has left a smaller count behind: its SSU is then read 6 bytes
    # past its end (zeros, as a Qt 5 QByteArray gives them)
    sus += isu_chain(aes[1], 0x88, 8, 1, b'OV' + b'ERLONG..', g.rng, nooct=14)[:1]
    sus += isu_chain(aes[1], 0x88, 8, 2, b'\x00\x00', g.rng, seqno=0)[:1]
    sus.append(make_su([0xC0, 0x81] + list(b'ERLONG..')))
    sus += isu_chain(0, 0x87, 7, 7, acars_ud(text='AES ZERO'), g.rng)
    return sus


def acars_path_sus(g, expiry=True):
    """the cases of PChannelHost::parse and ::defragment"""
    a = g.aes[6]
    kw = dict(aes=a, ges=0x90, reg='.D-ABCD', label='H1')
    sus = []
    sus += g.acars('REG PARITY', bad=(6,), **kw)
    sus += g.acars('TEXT PARITY', bad=(20,), **kw)
    sus += g.acars(['D', 'E', 'L', 0x7F, 'X'], **kw)
    sus += g.acars('', stx=False, **kw)  # 19 bytes, ETX at byte 15: ACARS without text
    ud17 = acars_ud(reg='.D-ABCD', text='')[:16] + b'\x7f'
    sus += isu_chain(a, 0x90, 1, 9, ud17[:16], g.rng)  # 16 bytes: not ACARS
    sus += isu_chain(a, 0x90, 1, 10, ud17, g.rng)  # 17 bytes: ACARS, byte 13 read as the terminator
    sus += isu_chain(a, 0x90, 1, 11, bytes(g.rand(30)), g.rng)  # non-ACARS hex
    # more-to-come chains: three blocks; block id wrapping Z -> A; a TAK mismatch
    for i, bi in enumerate('ABC'):
        sus += g.acars('PART %s ' % bi, bi=bi, more=i < 2, **kw)
    for i, bi in enumerate('YZA'):
        sus += g.acars('WRAP %s ' % bi, bi=bi, more=i < 2, **dict(kw, label='SA'))
    sus += g.acars('TAK ONE ', bi='A', more=True, tak=0x31, **dict(kw, label='Q0'))
    sus += g.acars('TAK TWO', bi='B', tak=0x32, **dict(kw, label='Q0'))
    if expiry:
        sus += acars_expiry_sus(g)
    return sus


def acars_expiry_sus(g):
    """a waiting fragment expires when its count passes 30, which the closing
    block itself takes part in: after 30 further ACARS items it is gone, after
    29 still there; the items between are the shortest ACARS there is (17
    bytes of user data, three SUs)"""
    kw = dict(aes=g.aes[6], ges=0x90, reg='.D-ABCD')
    short = acars_ud(reg='.N00000', label='10', text='')[:16] + b'\x7f'
    sus = []
    for label, first, n, last in (('B6', 'EXPIRES ', 30, 'TOO LATE'), ('5Z', 'KEPT ', 29, 'IN TIME')):
        sus += g.acars(first, bi='A', more=True, label=label, **kw)
        for j in range(n):
            sus += isu_chain(g.aes[7], 0x91, j & 15, j >> 4, short, g.rng)
        sus += g.acars(last, bi='B', label=label, **kw)
    return sus


def _uw_edit(kind, what):
    p = kind == 'p10500'
    return {'spoil': dict(uw=(UW ^ 1, UW ^ (1 << 17)) if p else UW ^ (1 << 9)),
            'none': dict(uw=(None, None) if p else None)}[what]


def _split_isu(kind, g, middle):
    """an ISU as the last SU of a frame, its SSUs in the next (`middle`: SUs put between them)"""
    per = KINDS[kind]['info'] // 12
    x = isu_chain(g.aes[0], 0x99, 9, 9, acars_ud(text='SPLIT OVER FRAMES'), g.rng)
    return [g.fill() for _ in range(per - 1)] + x[:1] + list(middle) + x[1:]


@functools.lru_cache(maxsize=None)
def shift_limits(kind):
    """uw_early / uw_late for 10500: frames shortened (d bits taken out of the
    dummy field) or lengthened (d seeded bits put in), searched with the untimed
    oracle.  Returns dict(early=last d whose UW still syncs at its place,
    block=last d whose block still completes before that UW, late=last d of a
    lengthened frame that still syncs)."""
    K = KINDS[kind]
    total = K['nbits']

    def syncs_at(d, sign):
        """the edited frame's UW gives a sync where it completes"""
        g = Grammar(11)
        edit = dict(remove=(20, d)) if sign < 0 else dict(insert=(20, d))
        s = Stream(kind, 'probe', [(g.frames(kind, 1)[0], edit)] + [(f, None) for f in g.frames(kind, 2)], gram=g)
        lt = run_oracle(kind, s.pcm)['trace']
        want = total - 1 - d if sign < 0 else d - 1
        sy = lt[(lt[:, 0] == tl.LK_SYNC) & (lt[:, 2] == want)]
        fr = len(sy) and ((lt[:, 0] == tl.LK_FRAME) & (lt[:, 1] <= sy[0, 1]) & (lt[:, 1] > sy[0, 1] - want - 1)).any()
        return bool(len(sy)), bool(fr)

    def last_true(f, lo, hi):
        assert f(lo) and not f(hi), 'the search interval does not bracket the limit'
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if f(mid) else (lo, mid)
        return lo

    if kind == 'p10500':
        early = last_true(lambda d: syncs_at(d, -1)[0], 1, 400)
        block = last_true(lambda d: syncs_at(d, -1)[1], 1, early)
        late = last_true(lambda d: syncs_at(d, +1)[0], 1, 40)
        return dict(early=early, block=block, late=late)
    # MSK's search is never gated: by one bit, as the issue names it
    assert syncs_at(1, -1)[0] and syncs_at(1, +1)[0]
    return dict(early=1, late=1)


def _drop(kind, g, a, b):
    """`a` frames without a UW whose SUs all fail, then `b` flywheel frames with good SUs"""
    per = KINDS[kind]['info'] // 12
    return [(_masked(kind, g, [False] * per), _uw_edit(kind, 'spoil')) for _ in range(a)] + \
           [(f, _uw_edit(kind, 'spoil')) for f in g.frames(kind, b)]


@functools.lru_cache(maxsize=None)
def lost_lengths(kind):
    """uw_lost: the fewest UW-less frames with failing SUs after which the
    ticked oracle drops datacd, and the fewest flywheel frames with good SUs
    after which its CRCs alone raise it again (no sync in between)"""
    for a in range(1, MAX_ADV - 2):
        for b in range(1, MAX_ADV - 1 - a):
            g = Grammar(5, a, b)
            s = Stream(kind, 'uw_lost', _drop(kind, g, a, b) + [(f, None) for f in g.frames(kind, 1)], gram=g)
            lt = adv_events(s, run_oracle(kind, s.pcm, tick=True)['trace'])
            ch = model_datacd(lt, True)
            if [c[2] for c in ch[:2]] == ['tick', 'crc']:
                return a, b
    raise AssertionError('%s: no drop / flywheel lengths make the CRCs raise datacd' % kind)


def _mix(kind, g):
    """eight frames whose SUs fail but for the last 0 .. 3 (seeded) and whose
    UW is spoiled (a sync would put the countdown back to 12), two good frames"""
    per = KINDS[kind]['info'] // 12
    good = [int(v) for v in g.rng.choice([0, 1, 1, 2, 2, 3], MAX_ADV - 2)]
    return [(_masked(kind, g, [k >= per - n for k in range(per)]), _uw_edit(kind, 'spoil')) for n in good] + \
           [(f, None) for f in g.frames(kind, 2)]


def mix_skip(kind, s):
    """the tick of a crc_mix stream's adversarial part on which the outcome
    hangs: without it the DataCarrierDetect changes or the frames differ
    (None: there is none).  Ticks that leave the countdown negative first."""
    good = run_oracle(kind, s.pcm, tick=True)
    lt = good['trace']
    tk = lt[lt[:, 0] == tl.LK_TICK]
    inside = np.nonzero(tk[:, 1] + lt_offset(s, lt) > s.adv_bit)[0]
    for k in sorted(inside, key=lambda k: (tk[k, 3] >= 0, k)):
        bad = run_oracle(kind, s.pcm, skip_tick=int(k))
        if bad['edges'] != good['edges'] or not np.array_equal(bad['frames'], good['frames']):
            return int(k)
    return None


@functools.lru_cache(maxsize=None)
def mix_pattern(kind):
    """crc_mix: seeded per-SU CRC patterns; the first seed with which the ticked
    oracle's ticks leave the countdown at -1 and at -2 and a later frame takes
    it above 2 again"""
    per = KINDS[kind]['info'] // 12
    for seed in range(64):
        g = Grammar(6, seed)
        adv = _mix(kind, g)
        s = Stream(kind, 'crc_mix', adv, gram=g)
        out = run_oracle(kind, s.pcm, tick=True)
        lt = out['trace']
        tk = lt[lt[:, 0] == tl.LK_TICK]
        neg = [int(v) for v in tk[:, 3] if v < 0]
        if -1 in neg and -2 in neg and out['edges'] > 1:
            last = max(tk[tk[:, 3] < 0][:, 1])
            if (lt[(lt[:, 0] == tl.LK_FRAME) & (lt[:, 1] > last)][:, 3] > 2).any() and mix_skip(kind, s) is not None:
                return seed
    raise AssertionError('%s: no seed takes the countdown to -1 and -2 at ticks' % kind)


@functools.lru_cache(maxsize=None)
def noisy_ebn0(kind):
    """the nominal Eb/N0 over the adversarial frames (in steps of 0.25 dB from
    5 dB down) at which between 25 % and 75 % of the oracle's SU CRCs in the
    six frames that carry them fail"""
    per = KINDS[kind]['info'] // 12
    for e4 in range(20, -13, -1):
        g = Grammar(8)
        s = Stream(kind, 'noisy', [(f, None) for f in g.frames(kind, 6)], adv_ebn0=e4 / 4, gram=g)
        m = masks(run_oracle(kind, s.pcm))[-6:]
        share = sum(bin(x).count('1') for x in m) / float(per * max(1, len(m)))
        if len(m) == 6 and 0.25 <= share <= 0.75:
            return e4 / 4
    raise AssertionError('%s: no Eb/N0 gives a mask share between 25 %% and 75 %%' % kind)


P_CLASSES = ('plain', 'su_types', 'crc_zero', 'crc_mix', 'uw_lost', 'uw_inverted', 'uw_one_arm', 'uw_skew',
             'uw_early', 'uw_late', 'uw_in_data', 'uw_in_data_drop', 'header_lo', 'header_hi', 'isu_paths',
             'isu_split', 'acars_paths', 'acars_expiry', 'noisy')
MSK_CLASSES = ('plain', 'su_types', 'crc_zero', 'crc_mix', 'uw_missing', 'uw_in_data1', 'uw_in_data2', 'uw_train',
               'uw_early', 'uw_late', 'isu_paths')
# the classes whose point is the DCD timer (the rest run with it as well)
TICK_CLASSES = ('crc_mix', 'uw_lost', 'uw_in_data_drop', 'uw_train')


def classes(kind):
    return P_CLASSES if kind == 'p10500' else MSK_CLASSES


@functools.lru_cache(maxsize=None)
def stream(kind, name):
    K = KINDS[kind]
    per = K['info'] // 12
    g = Grammar(2, K['bitrate'], sum(name.encode()))
    plain = lambda n: [(f, None) for f in g.frames(kind, n)]
    ebn0 = None
    if name == 'plain':
        adv = plain(6)
    elif name == 'su_types':
        adv = _su_types(kind, g)
    elif name == 'crc_zero':
        adv = _crc_zero(kind, g)
    elif name == 'crc_mix':
        g = Grammar(6, mix_pattern(kind))
        adv = _mix(kind, g)
    elif name == 'uw_lost':
        a, b = lost_lengths(kind)
        g = Grammar(5, a, b)
        adv = _drop(kind, g, a, b) + [(f, None) for f in g.frames(kind, 1)]
    elif name == 'uw_missing':  # MSK: three flywheel frames
        adv = plain(2) + [(f, _uw_edit(kind, 'spoil')) for f in g.frames(kind, 3)] + plain(2)
    elif name == 'uw_inverted':  # a polarity change on both arms, then on one, then true again
        adv = plain(1) + [(g.frames(kind, 1)[0], dict(pol=(True, True)))] + plain(1) + \
              [(g.frames(kind, 1)[0], dict(pol=(True, False)))] + plain(1) + \
              [(g.frames(kind, 1)[0], dict(pol=(False, True)))] + plain(1) + \
              [(g.frames(kind, 1)[0], dict(pol=(False, False)))] + plain(2)
    elif name == 'uw_one_arm':
        adv = plain(1) + [(g.frames(kind, 1)[0], dict(uw=(UW, None)))] + plain(2) + \
              [(g.frames(kind, 1)[0], dict(uw=(None, UW)))] + [(g.frames(kind, 1)[0], dict(uw=(None, UW)))] + plain(2)
    elif name == 'uw_skew':
        # the I arm's UW one arm symbol early: both detectors hit one bit apart in the other order;
        # two symbols early: the hits lie three bits apart and never pair
        adv = plain(1) + [(g.frames(kind, 1)[0], dict(skew_i=-1))] + plain(2) + \
              [(g.frames(kind, 1)[0], dict(skew_i=-2))] + plain(3)
    elif name in ('uw_early', 'uw_late'):
        lim = shift_limits(kind)
        if name == 'uw_early' and kind == 'p10500':
            ds = [lim['block'], lim['block'] + 1, lim['early'], lim['early'] + 1]
            adv = []
            for d in ds:
                adv += [(g.frames(kind, 1)[0], dict(remove=(20, d)))] + plain(1)
            adv += plain(1)
        elif name == 'uw_early':
            adv = plain(1) + [(g.frames(kind, 1)[0], dict(remove=(20, 1)))] + plain(2) + \
                  [(g.frames(kind, 1)[0], dict(remove=(K['hdr'] + 400, 1)))] + plain(2)
        elif kind == 'p10500':
            adv = plain(1) + [(g.frames(kind, 1)[0], dict(insert=(20, lim['late'])))] + plain(2) + \
                  [(g.frames(kind, 1)[0], dict(insert=(20, lim['late'] + 1)))] + plain(3)
        else:
            adv = plain(1) + [(g.frames(kind, 1)[0], dict(insert=(20, 1)))] + plain(2) + \
                  [(g.frames(kind, 1)[0], dict(insert=(K['hdr'] + 400, 1)))] + plain(2)
    elif name in ('uw_in_data', 'uw_in_data_drop'):
        # a doubled UW (both arms, twice) over the middle of the data area
        two = np.repeat(np.concatenate([uw_bits(UW), uw_bits(UW)]), 2)
        hit = (g.frames(kind, 1)[0], dict(write=[(K['hdr'] + 2400, two)]))
        if name == 'uw_in_data':
            adv = plain(1) + [hit] + plain(2) + [(g.frames(kind, 1)[0], dict(write=[(K['hdr'] + 2401, two)]))] + plain(2)
        else:
            gd = Grammar(5, drop_frames(kind))
            adv = _drop(kind, gd, drop_frames(kind), 0) + [hit] + plain(2)
    elif name in ('uw_in_data1', 'uw_in_data2'):  # MSK: a UW that ends the frame's first / second block
        B = 64 * K['N']
        # 1: a UW 8 bits into block 2, then one that ends on block 1's last bit;
        # 2: a UW that ends on block 2's last bit (N = 9: the frame's last data bit)
        ats = (K['hdr'] + B + 8, K['hdr'] + B - 32) if name == 'uw_in_data1' else (K['hdr'] + 2 * B - 32,) * 2
        adv = plain(1) + [(g.frames(kind, 1)[0], dict(write=[(ats[0], uw_bits(UW))]))] + plain(3) + \
              [(g.frames(kind, 1)[0], dict(write=[(ats[1], uw_bits(UW))]))] + plain(3)
    elif name == 'uw_train':  # MSK: twelve UWs back to back over the data area, twice
        train = np.concatenate([uw_bits(UW)] * 12)
        adv = plain(1) + [(g.frames(kind, 1)[0], dict(write=[(K['hdr'] + 100, train)]))] + plain(2) + \
              [(g.frames(kind, 1)[0], dict(write=[(K['hdr'] + 500, train)], uw=None))] + plain(3)
    elif name in ('header_lo', 'header_hi'):
        adv = _header(kind, g, range(0, 8) if name == 'header_lo' else range(8, 16))
    elif name == 'isu_paths':
        adv = [(f, None) for f in g.pack(kind, isu_path_sus(g, long=kind == 'p10500'))]
    elif name == 'isu_split':
        # clean; over a shortened frame (its early UW resets the ISUs); over eleven other ISUs
        others = [isu_chain(g.aes[0], 0x99, 6, j, b'\x00\x00', g.rng, seqno=0)[0] for j in range(11)]
        lim = shift_limits(kind)
        a, b, c = (g.pack(kind, _split_isu(kind, g, m)) for m in ([], [], others))
        adv = [(f, None) for f in a] + [(b[0], None), (b[1], dict(remove=(20, lim['block'])))] + \
              [(f, None) for f in b[2:]] + [(f, None) for f in c]
    elif name == 'acars_paths':
        adv = [(f, None) for f in g.pack(kind, acars_path_sus(g, expiry=False))]
    elif name == 'acars_expiry':
        adv = [(f, None) for f in g.pack(kind, acars_expiry_sus(g))]
    elif name == 'noisy':
        g = Grammar(8)
        return Stream(kind, name, [(f, None) for f in g.frames(kind, 6)], adv_ebn0=noisy_ebn0(kind), gram=g)
    else:
        raise KeyError(name)
    return Stream(kind, name, adv, ebn0=ebn0, gram=g)


@functools.lru_cache(maxsize=None)
def reference(kind, name, schedule='12000', tick=False):
    return run_oracle(kind, stream(kind, name).pcm, schedule, tick, per_run=True)
