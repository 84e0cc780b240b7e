"""The Viterbi input set (tests/viterbi_inputs.py) bites: for every rule that
makes a decoder equal to the oracle, the oracle's decoder with that rule
broken (oracle_viterbi_decode_soft_mut) decodes some stream of the set
differently, at every codeword length where the rule can decide a bit.  So a
device decoder wrong in one of these ways fails tests/test_gpu_viterbi.py,
which feeds it the same bytes."""
import numpy as np
import pytest

import viterbi_inputs as vi

ACS_TIE, SEARCH_TIE, NO_RENORM, TB_STATE0, TAIL_UNRESTRICTED = 1, 2, 3, 4, 5


def _tail_traceback_lengths():
    """Lengths at which a windowed traceback (140 columns held, then every 105)
    falls on one of the last 6 steps, whose search is restricted."""
    return [n for n in vi.LENGTHS if any(t > vi.columns(n) - 6 for t in vi.windowed_tracebacks(n))]


def _matters(mut, nsoft):
    if mut == ACS_TIE:
        return True
    if mut in (SEARCH_TIE, TB_STATE0):  # only a windowed traceback starts from a searched state
        return bool(vi.windowed_tracebacks(nsoft))
    if mut == NO_RENORM:
        # the longest R/T block and the OQPSK and C blocks.  At the short
        # lengths the metrics never wrap, so the subtraction changes no
        # compare: nothing is asserted there.
        return nsoft in (max(vi.RT_LENGTHS),) + vi.BLOCK_LENGTHS[4992] + vi.C_LENGTHS
    return nsoft in _tail_traceback_lengths()


def _detected(mut, nsoft):
    names, rows = vi.streams(nsoft)
    ref = vi.oracle_bits(nsoft)
    for i in reversed(range(len(names))):  # the fixed streams first: all128 alone shows the tie rules
        if not np.array_equal(vi.oracle_decode(rows[i], mut), ref[i]):
            return names[i]
    return None


def test_schedule_lengths():
    assert [n for n in vi.LENGTHS if not vi.windowed_tracebacks(n)] == [128]
    assert _tail_traceback_lengths() == [512, 2816, 5546]
    assert [n for n in vi.LENGTHS if _matters(NO_RENORM, n)] == [5016, 5078, 5484, 5546, 6080]
    assert len(vi.LENGTHS) == 40 and max(vi.LENGTHS) == 6080


def test_streams_are_what_they_say(cpu_libs):
    for nsoft in (128, 470, 5546):
        names, rows = vi.streams(nsoft)
        assert rows.shape == (len(vi.SEEDED) * len(vi.SEEDS) + len(vi.FIXED), nsoft) and rows.dtype == np.uint8
        by = dict(zip(names, rows))
        assert set(np.unique(by['hard', 3])) == {0, 255} and set(np.unique(by['near128', 1])) == {127, 128, 129}
        assert set(np.unique(by['tern', 0])) == {0, 128, 255} and np.all(by['all128', 0] == 128)
        assert by['alt', 0][:4].tolist() == [0, 255, 0, 255]
        assert not np.array_equal(by['uniform', 0], by['uniform', 1])
        # a clean codeword decodes to its message, and the zero tail is part of it
        code, msg = vi.encoded_bits(np.random.default_rng(nsoft), nsoft, message=True)
        dec = vi.oracle_decode(code * 255)
        assert np.array_equal(dec[:len(msg)], msg) and not dec[len(msg):].any()
    # every event boundary carries a bursterr run at one of four seeds
    assert vi.burst_columns(6080) == [0, 64, 128, 140, 192, 245, 3031]
    assert vi.burst_columns(128) == [0, 55]


@pytest.mark.parametrize('mut,name', [(ACS_TIE, 'acs_tie'), (SEARCH_TIE, 'search_tie'), (NO_RENORM, 'no_renorm'),
                                      (TB_STATE0, 'traceback_from_state0'), (TAIL_UNRESTRICTED, 'tail_unrestricted')])
def test_mutation_changes_a_decoded_bit(cpu_libs, mut, name):
    missed = [n for n in vi.LENGTHS if _matters(mut, n) and _detected(mut, n) is None]
    assert not missed, '%s: no stream of the set shows it at lengths %s' % (name, missed)
