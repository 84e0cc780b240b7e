"""tests/survey_model.py on the CPU: the model's composition (conversion,
window, JFFT, power, bin order) against numpy.fft.fft, its carry across reads,
and its DC recurrence."""
import numpy as np
import pytest

import aero_testlib as tl
import survey_model as sm


@pytest.mark.parametrize('log2n', [12, 13, 14])
@pytest.mark.parametrize('window', ['none', 'hann'])
def test_model_agrees_with_numpy_fft(cpu_libs, log2n, window):
    """1e-9 of the largest bin: FP64 rounding at these sizes is six orders below that, a wrong
    bin order, window or conjugation is not."""
    n = 1 << log2n
    x = sm.stream('tones', nreads=2)
    w = sm.WINDOWS[window](n)
    acc, seg = sm.survey(x, log2n, w)
    assert seg == len(x) // n
    ref = np.zeros(n)
    for s in range(seg):
        v = x[s * n:(s + 1) * n].astype(np.complex128)
        ref += np.abs(np.fft.fft(v if w is None else v * w)) ** 2
    assert np.max(np.abs(acc - ref)) <= 1e-9 * np.max(ref)
    k = int(np.argmax(acc))  # the strongest tone, 21500 Hz above the centre, is in the lower half
    assert abs(k * 288000.0 / n - 21500.0) <= 288000.0 / n


@pytest.mark.parametrize('log2n', [12, 13, 14])
def test_carry_does_not_depend_on_the_cut(cpu_libs, log2n):
    x = sm.stream('tones', nreads=3)
    whole = sm.survey(x, log2n)
    m = sm.SurveyModel(log2n)
    for b in range(3):
        m.feed(x[b * sm.B288:(b + 1) * sm.B288])
        assert len(m.carry) == ((b + 1) * sm.B288) % (1 << log2n) > 0  # no read ends on the grid
    acc, seg = m.read()
    assert seg == whole[1] and np.array_equal(acc.view(np.uint64), whole[0].view(np.uint64))
    ragged = sm.SurveyModel(log2n)
    for part in tl.cut(x, (1, 4095, 4097, 20000, 3)):
        ragged.feed(part)
    assert np.array_equal(ragged.read()[0].view(np.uint64), whole[0].view(np.uint64))


def test_reset_keeps_the_grid(cpu_libs):
    x = sm.stream('tones', nreads=3)
    m = sm.SurveyModel(12)
    m.feed(x[:sm.B288])
    first, s1 = m.read(reset=True)
    m.feed(x[sm.B288:])
    second, s2 = m.read()
    assert s1 == 14 and s1 + s2 == 3 * sm.B288 // 4096
    a = np.zeros(4096)
    for s in range(s1, s1 + s2):
        a = a + sm.segment_power(x[s * 4096:(s + 1) * 4096], None)
    assert np.array_equal(second.view(np.uint64), a.view(np.uint64))


def test_dc_removal_recurrence(cpu_libs):
    """dc_remove: its state carries from call to call and its first step is demodData's
    expression in float32 (tests/test_gpu_survey.py holds it against dc_kernel's output)."""
    x = sm.stream('dc', nreads=7)[:4000]
    state = [np.float32(0), np.float32(0)]
    y = np.concatenate([sm.dc_remove(x[:1500], state), sm.dc_remove(x[1500:], state)])
    assert np.array_equal(y.view(np.uint32), sm.dc_remove(x).view(np.uint32))  # the state carries
    k1 = np.float32(1.0) - np.float32(0.000001)
    a = np.float32(0) * k1 + np.float32(0.000001) * x[0].real
    assert y[0].real == x[0].real - a
    assert abs(np.mean(x).real - 0.125) < 0.01 and abs(np.mean(y).real - 0.125) < 0.01  # 4000 samples barely move it
