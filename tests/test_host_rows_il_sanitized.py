"""libfpcc_host's interleaved row coder under AddressSanitizer + UBSan, as a stand-alone program (tests/host/rows_il_checks.cpp) built
from fastpcc_amd/csrc/host/rans_host.cpp and its own main with the sanitizer runtimes linked statically, and run as a child process:
round trips over the size / (a, b) / row width grid, the default policy, hostile headers, payloads and rows, the encoder's refusals.
Nothing is loaded into Python under a sanitizer.

CPU only: the module is skipped where a GPU is visible (sanitizer programs do not belong on the shared GPU machines)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SRC = os.path.join(ROOT, 'fastpcc_amd', 'csrc', 'host', 'rans_host.cpp')
CHECKS_SRC = os.path.join(ROOT, 'tests', 'host', 'rows_il_checks.cpp')
BASE = ['-O1', '-g', '-fno-omit-frame-pointer']
CXX = ['-std=c++17', '-pthread', '-march=x86-64-v3', '-Wall', '-Wextra']          # as _build.build_host
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
LINK = ['-static-libasan', '-static-libubsan']
REPORTS = ('runtime error:', 'ERROR: AddressSanitizer')


def _has_gpu():                                   # the test tests/conftest.py uses
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


pytestmark = pytest.mark.skipif(_has_gpu(), reason='sanitizer programs run on the CPU machine only')


def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('host_rows_il_sanitized'))
    if not (shutil.which('g++') and shutil.which('timeout')):
        pytest.skip('no g++ / timeout')
    probe = os.path.join(tmp, 'probe.cpp')
    with open(probe, 'w') as f:
        f.write('#include <cstdio>\nint main(int c, char **) { int *p = new int[4]; p[0] = c; std::printf("%d\\n", p[0] + 2); delete[] p; return 0; }\n')
    out = _run(['g++'] + BASE + SANITIZE + LINK + CXX + [probe, '-o', probe[:-4]], timeout=300)
    if out.returncode != 0:
        pytest.skip('a trivial -fsanitize program does not build: ' + out.stdout[-300:])
    out = _run(['timeout', '-k', '5', '60', probe[:-4]], timeout=90)
    if out.returncode != 0 or out.stdout.strip() != '3':
        pytest.skip('a trivial -fsanitize program does not run: ' + out.stdout[-300:])
    exe = os.path.join(tmp, 'rows_il_checks_asan')
    out = _run(['g++'] + BASE + SANITIZE + LINK + CXX + [CHECKS_SRC, HOST_SRC, '-o', exe], timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    return exe


def test_rows_il_checks_under_asan_and_ubsan(program):
    out = _run(['timeout', '-k', '10', '300', program], timeout=330)
    text = out.stdout
    print(text[-6000:])
    assert not [line for line in text.splitlines() if any(r in line for r in REPORTS)], text[-4000:]
    assert out.returncode == 0, text[-4000:]
    assert not [line for line in text.splitlines() if ': FAIL' in line]
    listed = _run([program, '--list'], timeout=60).stdout.split()
    assert len(listed) >= 5 and all('%s: ok' % name in text for name in listed)
