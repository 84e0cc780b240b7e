"""What tests/test_gpu_msg_paths.py relies on, checked with the oracle alone.

Its channeliser case can tell a feed that fuses the reads of a batch into one
message from one that delivers a message per read only if the oracle's output
on that very audio depends on the cut: the soft bits of the C channel and of
the burst channel differ between one-read and two-read messages.  And every
oracle the GPU cases compare with decoded frames, SUs and voice frames (R/T
packets), so no comparison is between two empty outputs."""
import numpy as np

import aero_testlib as tl
import oracle_tick as ot
import test_gpu_msg_paths as mp


def test_channeliser_audio_tells_the_message_cut(cpu_libs):
    _, audio, _, spb = tl.boundary_input()
    assert spb == [9600, 9600] and all(len(a) == 480000 for a in audio)
    one, two = (tl.c_reference(tl.cut(audio[0], (k * spb[0],))) for k in (1, 2))
    assert tl.c_produced(one) and len(one['soft']) > 10000
    assert not np.array_equal(one['soft'], two['soft']), 'the C audio does not tell one-read from two-read messages'
    assert not np.array_equal(one['frames'], two['frames'])
    for tick in (True, False):
        b1, b2 = (ot.run(audio[1], k * spb[1], tick=tick) for k in (1, 2))
        assert len(b1['packets']) >= 2 and len(b1['soft']) > 1000
        assert not np.array_equal(b1['soft'], b2['soft']), 'the burst audio does not tell the message cut'


def test_plain_streams_tell_the_message_cut(cpu_libs):
    c = tl.synth_c(seconds=6.0, seed=0xC1A5, carrier=11000.0, ebn0=12.0)
    one, two = (tl.c_reference(tl.cut(c, (n,))) for n in (12000, 24000))
    assert (len(one['soft']), len(two['soft'])) == (48224, 43040)
    b = tl.synth_burst(seconds=10.0, seed=0xAE50)
    assert [len(ot.run(b, n, tick=False)['soft']) for n in (12000, 24000)] == [12005, 15845]


def test_gpu_cases_are_not_vacuous(cpu_libs):
    refs = mp.build_refs()
    assert len(refs) == 7
    for key, r in refs.items():
        assert tl.c_produced(r) and len(r['soft']) > 10000 and len(r['hops']) > 0 and len(r['pt']) > 0, key
    r = refs[(0, 12000)]
    assert (len(r['soft']), len(r['frames']), len(r['c_units']), len(r['voice']), len(r['hops'])) == \
        (48224, 1920, 7, 6, 70)
    r = refs[(0, 'ragged')]
    assert (len(r['soft']), len(r['frames']), len(r['c_units']), len(r['voice'])) == (47072, 1600, 5, 5)
    r = refs['B']
    assert (len(r['frames']), len(r['c_units']), len(r['voice'])) == (1920, 4, 6)
