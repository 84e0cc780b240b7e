"""bin/aero-publish with the [General] survey keys: on a CF32 file of 8 reads
at 288 ksps with three tones it logs the three carriers, with the frequencies
aero_survey_peaks gives on the model's spectrum (tests/survey_model.py) of the
same reads; with the keys absent its log holds no survey line."""
import math
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import aero_testlib as tl
import survey_model as sm

pytestmark = pytest.mark.gpu

BIN = os.path.join(tl.ROOT, 'aero-cli_amd', 'bin')
C = tl.CENTER
FS = 288000
LINE = re.compile(r'^survey: carrier (-?\d+) Hz bandwidth (\d+) Hz ratio (\S+) vfo (\S+)$')


def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _ini(vfos, extra=()):
    cfg = dict(sample_rate=FS, center_frequency=C, mains=[dict(frequency=C, out_rate=FS)], vfos=vfos)
    text = tl.c5_ini(cfg).replace('tcp://*:6004', 'tcp://127.0.0.1:%d' % _free_port())
    return text.replace('correct_dc_bias=0', '\n'.join(('correct_dc_bias=0',) + tuple(extra)))


def _publish(tmp_path, x, ini_text):
    wb, ini = tmp_path / 'wideband.cf32', tmp_path / 'survey.ini'
    x.astype(np.complex64).tofile(str(wb))
    ini.write_text(ini_text)
    r = subprocess.run([os.path.join(BIN, 'aero-publish'), '-d', 'driver=file,path=%s' % wb, str(ini)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr.splitlines()


def test_survey_lines(engine_lib, cpu_libs, tmp_path):
    import build
    import aero_engine as ae
    build.build_host()
    x = sm.stream('tones', nreads=8)
    # the entry at the 91-kHz carrier is inside its band, the others are 1 to 1.5 kHz off theirs
    vfos = [dict(frequency=C + 20000, data_rate=10500, gain=100.0), dict(frequency=C - 50000, data_rate=600, gain=100.0),
            dict(frequency=C + 91000, data_rate=1200, gain=100.0)]
    lines = _publish(tmp_path, x, _ini(vfos, ('survey_log2n=12', 'survey_period=4', 'survey_threshold=10',
                                              'survey_min_bins=2')))
    got = [LINE.match(l).groups() for l in lines if l.startswith('survey:')]
    # the binary's window: the C library's cos, as Python's math.cos
    w = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * i / 4096) for i in range(4096)])
    m = sm.SurveyModel(12, w)
    want = []
    for half in (x[:4 * sm.B288], x[4 * sm.B288:]):  # a report with reset every 4 reads, the grid goes on
        m.feed(half)
        acc, seg = m.read(reset=True)
        assert seg >= 56
        for p in ae.survey_peaks(acc, 12, FS, C, threshold=10.0, min_bins=2, merge_gap=2):
            want.append((str(p['frequency']), '%.0f' % p['bandwidth_hz'], '%.1f' % p['ratio'],
                         '2' if abs(p['frequency'] - (C + 91000)) < 200 else '-'))
    assert len(want) == 6 and [int(f) for f, *_ in want[:3]] == sorted(int(f) for f, *_ in want[:3])
    for (f, *_), (tone, _) in zip(want[:3], sorted(sm.TONES3)):
        assert abs(int(f) - (C + tone)) <= FS / 4096
    assert got == want


def test_no_survey_line_without_the_keys(engine_lib, tmp_path):
    import build
    build.build_host()
    x = sm.stream('tones', nreads=8)
    vfos = [dict(frequency=C + 20000, data_rate=10500, gain=100.0)]
    base = _publish(tmp_path, x, _ini(vfos))
    assert base == [] or not any('survey' in l for l in base)
    assert base == _publish(tmp_path, x, _ini(vfos, ('survey_log2n=0',)))
    # an unsupported size is refused at start-up
    wb, ini = tmp_path / 'wideband.cf32', tmp_path / 'bad.ini'
    ini.write_text(_ini(vfos, ('survey_log2n=11',)))
    p = subprocess.run([os.path.join(BIN, 'aero-publish'), '-d', 'driver=file,path=%s' % wb, str(ini)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and 'survey_log2n=11' in p.stderr
