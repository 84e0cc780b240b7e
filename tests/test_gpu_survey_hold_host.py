"""bin/aero-publish with the [General] key survey_hold_group: on `gated`
(tests/survey_hold_model.py) written as a CF32 file it logs, behind the
report's carrier lines, one burst line for the gated carrier, with the values
aero_survey_peaks and aero_survey_activity give on the model's arrays; its
carrier lines are those of a run without the key, and without the key there is
no burst line."""
import math
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import aero_testlib as tl
import survey_hold_model as hm
import survey_model as sm

pytestmark = pytest.mark.gpu

BIN = os.path.join(tl.ROOT, 'aero-cli_amd', 'bin')
C = tl.CENTER
FS = 288000
BURST = re.compile(r'^survey: burst (-?\d+) Hz bandwidth (\d+) Hz on (\S+) off (\S+) vfo (\S+)$')
KEYS = ('survey_log2n=12', 'survey_period=7')


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


# the entry at the gated carrier is inside its band, the other is 1.5 kHz off its carrier
VFOS = [dict(frequency=C + 20000, data_rate=10500, gain=100.0), dict(frequency=C + 60000, data_rate=1200, gain=100.0)]


def test_burst_lines(engine_lib, cpu_libs, tmp_path):
    import build
    import aero_engine as ae
    build.build_host()
    x = hm.gated()
    lines = _publish(tmp_path, x, _ini(VFOS, KEYS + ('survey_hold_group=4',)))
    survey = [l for l in lines if l.startswith('survey:')]
    got = [BURST.match(l).groups() for l in survey if l.startswith('survey: burst')]
    # the binary's window: the C library's cos, as Python's math.cos
    w = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * i / 4096) for i in range(4096)])
    m = hm.run_model(x, 12, 4, 0, None, w)  # one report with reset after the 7 reads
    acc, seg = m.read()
    peak, low, _, groups = m.hold.read()
    assert seg == 98 and groups == 24
    runs = ae.survey_peaks(peak, 12, FS, C)
    acts = ae.survey_activity(acc, seg, peak, low, None, groups, 4, 12, 8.0, runs)
    want = [(str(p['frequency']), '%.0f' % p['bandwidth_hz'], '%.1f' % a['on_ratio'], '%.1f' % a['off_ratio'],
             '1' if abs(p['frequency'] - (C + 60000)) < 200 else '-')
            for p, a in zip(runs, acts) if a['kind'] == ae.SURVEY_BURST]
    assert len(runs) == 3 and len(want) == 1 and want[0][4] == '1' and abs(int(want[0][0]) - (C + 60000)) <= FS / 4096
    assert got == want
    # behind the period's two carrier lines, which are those of a run without the key
    assert [l.split()[1] for l in survey] == ['carrier', 'carrier', 'burst']
    plain = _publish(tmp_path, x, _ini(VFOS, KEYS))
    assert [l for l in plain if l.startswith('survey:')] == survey[:2]
    assert not any('burst' in l for l in plain)


def test_hold_group_without_a_survey_is_ignored(engine_lib, tmp_path):
    import build
    build.build_host()
    x = hm.gated()[:2 * sm.B288]
    lines = _publish(tmp_path, x, _ini(VFOS, ('survey_hold_group=4',)))
    assert not any(l.startswith('survey:') for l in lines)
    assert len([l for l in lines if 'WARN' in l and 'survey_hold_group' in l]) == 1
    assert not any('survey' in l for l in _publish(tmp_path, x, _ini(VFOS, ('survey_hold_group=0',))))
