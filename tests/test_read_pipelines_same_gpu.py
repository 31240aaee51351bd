"""The eight read-level pipelines compute what they computed before their Python layer was shared: every key of every result in its
order, every array and every log line in full, against a record made on the device at commit e815bed
(tests/golden/read_pipelines/, read_pipelines_case.py).  That commit reproduced every field bit for bit over two runs, so every field is
compared with exact equality (an array of more than read_pipelines_case.HASH_ABOVE bytes through its SHA-256)."""
import json

import pytest

import read_pipelines_case as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def record():
    return C.load_record()


@pytest.fixture(scope='module')
def inputs():
    return C.inputs()


def test_the_record_covers_the_eight_pipelines_and_is_exact_throughout(record, inputs):
    arrays, meta = record
    assert list(meta['pipelines']) == [name for name, _ in C.pipelines(inputs)] and len(meta['pipelines']) == 8
    assert meta['unstable'] == [] and not set(arrays) & set(meta['sha256'])


@pytest.mark.parametrize('index', range(8))
def test_pipeline_is_the_recorded_one(index, record, inputs):
    ref, meta = record
    name, call = C.pipelines(inputs)[index]
    lines, keys, arrays = [], {}, {}
    C.flatten(call(lines.append), name, arrays, keys)
    want = meta['pipelines'][name]
    assert json.loads(json.dumps(keys)) == want['keys'] and list(keys) == list(want['keys'])       # the keys of every dict, in order
    assert lines == want['log']
    expected = {k for k in list(ref) + list(meta['sha256']) if k.split('/')[0] == name}
    assert set(arrays) == expected
    for k, a in arrays.items():
        if k in meta['sha256']:
            assert C.digest(a) == meta['sha256'][k], k
        else:
            assert C.same_bits(a, ref[k]), k
