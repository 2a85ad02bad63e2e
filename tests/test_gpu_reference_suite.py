"""The reference's OWN unit tests for the rows of SURVEY.md §8, run on the GPU box with
``backend.install()`` active (``-p tests._install_plugin``): their ``@withDevice`` / ``@withCUDA``
cases put HIP tensors through this package's kernels and judge the results with the assertions the
reference's authors wrote: every module of test/utils, test/nn/conv (all 60-odd conv layers — the
ones without a dedicated route ride on `MessagePassing._index_select` + `scatter`), test/nn/aggr
and test/nn/dense, plus test_edge_index, test_index and the BasicGNN models — incl. their hook,
explain and bipartite cases — and (later in round 6) what sits ON TOP of the path: every module of
test/nn/models, nn/pool, nn/norm, nn/functional, nn/kge, nn/attention, nn/unpool, the top-level
test/nn modules, test/explain, test/transforms, test/data, test/sampler and test/metrics (313
modules, 4,141 cases).

The same modules run once WITHOUT the backend in the same environment: a test only counts against
install() if it passes there (a handful of the reference's tests fail on their own with this torch
version, e.g. TorchScript of ``GATConv``; random-input ``allclose`` checks are re-run once).
The test modules are staged data (``oracle/make_ref.py``: packed from ``/root/reference/test``
into the git-ignored ``oracle/_ref`` archive), never edited."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(root, files, with_backend, extra=(), full=False, workers=None):
    """One pytest process per test module, `workers` at a time (the modules are CPU-heavy —
    TorchScript, 2,700 small cases — and independent; pytest-xdist cannot split them: their
    parametrisations are not collected in a stable order).  Returns (failed node ids, a summary
    line, the concatenated output)."""
    from concurrent.futures import ThreadPoolExecutor

    if workers is None:   # 4 threads per module process
        # (every module process opens the device, and so does this one: twelve side by side keep
        # the count of processes holding the GPU well below sixteen)
        workers = 12
    from oracle import make_ref
    ref = make_ref.import_reference()
    ref_root = os.path.dirname(os.path.dirname(os.path.abspath(ref.__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, ref_root]), OMP_NUM_THREADS='4',
               MKL_NUM_THREADS='4')    # (twelve processes side by side: no 128-thread pools each)
    env.pop('FULL_TEST', None)
    if full:
        env['FULL_TEST'] = '1'

    def one(path):
        cmd = [sys.executable, '-m', 'pytest', path, '-q', '-p', 'no:cacheprovider', '-rf',
               '--rootdir', root, '--confcutdir', root, '-c', os.devnull, *extra]
        if with_backend:
            cmd += ['-p', 'tests._install_plugin']
        res = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=root,
                             timeout=1700)
        return res.stdout + res.stderr

    with ThreadPoolExecutor(max_workers=workers) as pool:
        outs = list(pool.map(one, files))
    out = '\n'.join(outs)
    failed = set(re.findall(r'^(?:FAILED|ERROR) (\S+)', out, flags=re.M))
    counts = {k: sum(int(n) for n in re.findall(rf'(\d+) {k}', out))
              for k in ('passed', 'failed', 'skipped', 'deselected')}
    line = ', '.join(f'{v} {k}' for k, v in counts.items() if v) + f' in {len(files)} modules'
    return failed, line, out


def _names(node_ids):
    """`-k` expression selecting the test FUNCTIONS of these node ids."""
    return ' or '.join(sorted({re.sub(r'\[.*', '', t.split('::')[-1]) for t in node_ids}))


# The rows of SURVEY.md §8 themselves: every module of test/utils, test/nn/conv, test/nn/aggr,
# test/nn/dense + test_edge_index, test_index, test_basic_gnn (142 modules, ~3,450 cases, ~2 min).
# This is what `pytest -m gpu` runs by default; PYGAMD_REFERENCE_SUITE=full adds what sits on top
# of the path (nn/models, nn/pool, nn/norm, ..., explain, transforms, data, sampler, metrics: 313
# modules, 4,141 cases, ~4.5 min — profiles/r06_reference_suite.txt holds that run).
CORE = ('/utils/', '/nn/conv/', '/nn/aggr/', '/nn/dense/', '/test_edge_index.py', '/test_index.py',
        '/nn/models/test_basic_gnn.py')


@pytest.mark.timeout(3500)
def test_reference_test_modules_pass_with_the_backend_installed():
    """One pass over the staged modules WITH the backend; whatever fails is run again WITHOUT it (the
    reference's own failures with this torch version do not count) and once more with it (random
    inputs against default `allclose` tolerances).  The TorchScript-heavy FULL_TEST variants run
    on the CPU (tests/test_backend_install.py) — on the device box they triple the run time."""
    from oracle import make_ref
    root, files = make_ref.reference_tests()
    assert len(files) >= 290, len(files)
    full = os.environ.get('PYGAMD_REFERENCE_SUITE', 'core') == 'full'
    if not full:
        files = [f for f in files if any(c in '/' + os.path.relpath(f, root) for c in CORE)]
        assert len(files) >= 135, len(files)
    failed, line, out = _run(root, files, with_backend=True)
    m = re.search(r'(\d+) passed', line)
    assert m and int(m.group(1)) >= (3900 if full else 3300), line
    assert 'cuda:0' in out or not failed    # (ids of device cases carry the device name)
    new = sorted(failed)
    if new:
        own, _, _ = _run(root, files, with_backend=False, extra=('-k', _names(new)))
        new = sorted(set(new) - own)
    if new:
        again, _, out = _run(root, files, with_backend=True, extra=('-k', _names(new)))
        new = sorted(set(new) & again)
    assert not new, (f'{len(new)} reference tests fail only with the backend installed: {new}\n'
                     f'installed: {line}\n' + out[-6000:])
    print('installed:', line)
    print('failing with AND without the backend (the reference\'s own, on this torch / box):',
          sorted(failed))
