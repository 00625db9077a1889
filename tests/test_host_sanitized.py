"""libfpcc_host's coders under the sanitizers, as stand-alone programs (tests/host/*.cpp): the rest of the suite reaches the library
through ctypes inside Python, where no sanitizer sees it.  The programs are built here from fastpcc_amd/csrc/host/rans_host.cpp, the
test oracle oracle/rans.c and their own main, with the sanitizer runtimes linked statically, and run as child processes:

    coder_checks   AddressSanitizer + UBSan   golden replay, differential against the oracle, exact-fit buffers, error paths, hostile streams
    pool_checks    AddressSanitizer + UBSan,  the background pool under flag-gated hand-over, the row warmers of the 255-ary decoder
                   and ThreadSanitizer        (FPCC_HOST_WARMERS = 0, 1, 4: read once per process)

CPU only: the module is skipped where a GPU is visible (sanitizer programs do not belong on the shared GPU machines)."""
import concurrent.futures
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SRC = os.path.join(ROOT, 'fastpcc_amd', 'csrc', 'host', 'rans_host.cpp')
ORACLE_SRC = os.path.join(ROOT, 'oracle', 'rans.c')
BASE = ['-O1', '-g', '-fno-omit-frame-pointer']
CXX = ['-std=c++17', '-pthread', '-march=x86-64-v3', '-Wall', '-Wextra']          # as _build.build_host
KINDS = {
    'asan': (['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], ['-static-libasan', '-static-libubsan']),
    'tsan': (['-fsanitize=thread'], ['-static-libtsan']),
}
REPORTS = ('runtime error:', 'ERROR: AddressSanitizer', 'WARNING: ThreadSanitizer')


def _has_gpu():                                   # the test tests/conftest.py uses
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


pytestmark = pytest.mark.skipif(_has_gpu(), reason='sanitizer programs run on the CPU machine only')


def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)


def _compile(cmd):
    out = _run(cmd, timeout=600)
    assert out.returncode == 0, ' '.join(cmd) + '\n' + out.stdout[-4000:]


def _sanitizer_works(kind, tmp):
    """None if a trivial threaded program with this sanitizer builds and runs clean, else the reason"""
    if not (shutil.which('g++') and shutil.which('gcc') and shutil.which('timeout')):
        return 'no g++ / gcc / timeout'
    flags, link = KINDS[kind]
    src = os.path.join(tmp, 'probe_%s.cpp' % kind)
    with open(src, 'w') as f:
        f.write('#include <cstdio>\n#include <thread>\nint main(int c, char **) { int *p = new int[4]; p[0] = c; std::thread t([p] { p[1] = 2; }); t.join();'
                ' std::printf("%d\\n", p[0] + p[1]); delete[] p; return 0; }\n')
    exe = os.path.join(tmp, 'probe_%s' % kind)
    out = _run(['g++'] + BASE + flags + link + CXX + [src, '-o', exe], timeout=300)
    if out.returncode != 0:
        return 'a trivial -fsanitize program does not build: ' + out.stdout[-300:]
    out = _run(['timeout', '-k', '5', '60', exe], timeout=90)
    if out.returncode != 0 or out.stdout.strip() != '3':
        return 'a trivial -fsanitize program does not run: ' + out.stdout[-300:]
    return None


@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    """{'coder_asan': path, 'pool_asan': path, 'pool_tsan': path}; the objects of all three are compiled side by side"""
    tmp = str(tmp_path_factory.mktemp('host_sanitized'))
    for kind in KINDS:
        why = _sanitizer_works(kind, tmp)
        if why:
            pytest.skip('%s: %s' % (kind, why))
    objs, jobs = {}, []
    for kind, (flags, _) in KINDS.items():
        for name, src in (('oracle', ORACLE_SRC), ('host', HOST_SRC), ('pool', os.path.join(ROOT, 'tests', 'host', 'pool_checks.cpp')),
                          ('coder', os.path.join(ROOT, 'tests', 'host', 'coder_checks.cpp'))):
            if name == 'coder' and kind != 'asan':
                continue
            obj = objs[name, kind] = os.path.join(tmp, '%s_%s.o' % (name, kind))
            cc = ['gcc'] + BASE + flags if src.endswith('.c') else ['g++'] + BASE + flags + CXX
            jobs.append(cc + ['-c', src, '-o', obj])
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(_compile, jobs))
    out = {}
    for prog, kind in (('coder', 'asan'), ('pool', 'asan'), ('pool', 'tsan')):
        flags, link = KINDS[kind]
        exe = out['%s_%s' % (prog, kind)] = os.path.join(tmp, '%s_checks_%s' % (prog, kind))
        _compile(['g++'] + flags + link + ['-pthread', objs[prog, kind], objs['host', kind], objs['oracle', kind], '-o', exe])
    out['tmp'] = tmp
    return out


def _ints(a):
    return ' '.join(str(int(v)) for v in np.asarray(a).reshape(-1))


def _floats(a):
    return ' '.join(float(v).hex() for v in np.asarray(a, dtype=np.float64).reshape(-1))


def _flat_golden(golden_dir, path):
    """tests/golden/rans.json and rans_random.json as the token file coder_checks reads; returns the number of cases per record kind"""
    with open(os.path.join(golden_dir, 'rans.json')) as f:
        G = json.load(f)
    with open(os.path.join(golden_dir, 'rans_random.json')) as f:
        R = json.load(f)
    assert set(G) == {'cdf', 'indexed', 'binary', 'simple'} and set(R) == {'cases'}        # a new section needs a replay of its own
    out, count = [], {}

    def record(kind, *lines):
        out.extend((kind + ' ' + lines[0],) + lines[1:] + ('end',))
        count[kind] = count.get(kind, 0) + 1

    for c in G['cdf']:
        pmf = np.array(c['pmf'], dtype=np.float64)
        record('cdf', '%d %d %d %d' % (c['overflow'], c['offset_in'], pmf.shape[0], pmf.shape[1]), _floats(pmf), _ints(c['offset_out']),
               *['%d %s' % (len(row), _ints(row)) for row in c['cdf']])
    for c in G['indexed']:
        record('indexed', '%d %d %d %d' % (c['overflow'], c['with_indexes'], len(c['cdfs']), len(c['symbols'])),
               *['%d %s' % (len(row), _ints(row)) for row in c['cdfs']], _ints(c['offsets']), _ints(c['symbols']), _ints(c['indexes']), c['stream'])
    for c in G['binary']:
        prob = np.array(c['prob']).reshape(-1)
        record('binary', '%d' % prob.size, _ints(prob), _ints(c['bits']), c['stream'])
    for c in G['simple']:
        if 'bin' in c:
            record('simplebin', '%d %d' % (len(c['bin']['edge']), len(c['bin']['bits'])), _ints(c['bin']['edge']), _ints(c['bin']['bits']), c['stream'])
            continue
        lines = []
        for blk in c['blocks']:
            rows = np.array(blk['rows'])
            lines += ['%d %d %d' % (rows.shape[0], rows.shape[1], len(blk['symbols'])), _ints(rows), _ints(blk['symbols'])]
        record('simple', '%d' % len(c['blocks']), *lines, c['stream'])
    for c in R['cases']:
        assert len(c['cdfs']) == 1
        record('random', '%d' % len(c['prob']), _ints(c['prob']), c['bits'], c['binary'], '%d' % len(c['hist']), _floats(c['hist']), '%d' % c['offset'],
               _ints(c['symbols']), '%d %s' % (len(c['cdfs'][0]), _ints(c['cdfs'][0])), c['indexed'])
    assert sum(count.values()) == sum(len(v) for v in G.values()) + len(R['cases'])
    with open(path, 'w') as f:
        f.write('\n'.join(out) + '\n')
    return count


def _checked(cmd, seconds, env=None):
    out = _run(['timeout', '-k', '10', str(seconds)] + cmd, timeout=seconds + 30, env=env)
    text = out.stdout
    print(text[-6000:])
    assert not [line for line in text.splitlines() if any(r in line for r in REPORTS)], text[-4000:]
    assert out.returncode == 0, text[-4000:]
    assert not [line for line in text.splitlines() if ': FAIL' in line]
    return text


def test_coder_checks_under_asan_and_ubsan(programs, golden_dir):
    flat = os.path.join(programs['tmp'], 'golden.txt')
    want = _flat_golden(golden_dir, flat)
    text = _checked([programs['coder_asan'], flat], 300)
    got = {}
    for line in text.splitlines():
        if line.startswith('replayed '):
            _, kind, n = line.split()
            got[kind] = int(n)
    assert got == want and all(n > 0 for n in want.values())          # every case of every section, none skipped
    listed = _run([programs['coder_asan'], '--list'], timeout=60).stdout.split()
    assert listed and all('%s: ok' % name in text for name in listed)


@pytest.mark.parametrize('warmers', ['0', '1', '4'])
@pytest.mark.parametrize('kind', ['asan', 'tsan'])
def test_pool_checks(programs, kind, warmers):
    text = _checked([programs['pool_%s' % kind]], 300, env=dict(os.environ, FPCC_HOST_WARMERS=warmers))
    assert 'FPCC_HOST_WARMERS=%s' % warmers in text
    for name in ('pool_two_contexts', 'warmers_one_thread', 'warmers_two_threads'):
        assert '%s: ok' % name in text
