"""CPU checks of tests/_caps1d.py, which tests/test_caps1d_gpu.py builds on: the cap is the literal of csrc/spikes_common.h and the six
launches that module covers are the only ones that use it, every shape lands in the regime its test claims -- a later change of a
shape or of the cap cannot quietly fall back to one trip per thread --, the lone second-trip item of the cap + 1 cases is the one
the tests say it is, and no buffer of a case reaches 256 MB."""
import os
import re

import numpy as np
import pytest

import _caps1d as c1

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'deep_calcium_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _entry_body(src, name):
    m = re.search(r'^extern "C" int %s\(.*?^}' % re.escape(name), src, flags=re.M | re.S)
    assert m, name
    return m.group(0)


def test_the_cap_is_the_one_the_source_states():
    common = _read('spikes_common.h')
    m = re.search(r'static inline int spikes_blocks\(long total, int cap = (\d+)\) \{\n(.*?)\n\}', common, flags=re.S)
    assert m and int(m.group(1)) == c1.CAP_BLOCKS == 8192
    assert 'const long b = (total + 255) / 256;' in m.group(2) and 'b > cap ? cap : b' in m.group(2)
    assert c1.THREADS == 256 and c1.CAP_ITEMS == 2097152
    assert c1.blocks(0) == 1 and c1.blocks(257) == 2 and c1.blocks(c1.CAP_ITEMS) == c1.blocks(10 ** 9) == 8192


def test_the_six_launches_are_the_only_users_of_the_cap():
    users = []
    for name in sorted(os.listdir(CSRC)):
        if not os.path.isfile(os.path.join(CSRC, name)):
            continue
        src = _read(name)
        for m in re.finditer(r'spikes_blocks\(', src):
            if name == 'spikes_common.h' and src[:m.start()].endswith('static inline int '):
                continue                                                  # the definition
            users.append((name, m.start()))
    assert len(users) == len(c1.LAUNCHES) == 6, users
    seen = []
    for entry, (kernel, fname) in c1.LAUNCHES.items():
        body = _entry_body(_read(fname), entry)
        # the default cap, 256 threads, and `total` as this module computes it
        assert re.search(r'hipLaunchKernelGGL\(%s, dim3\(spikes_blocks\(total\)\), dim3\(256\), 0,' % kernel, body), entry
        assert body.count('spikes_blocks(') == 1
        seen.append(fname)
        per = {'dc_maxpool1d_2_fwd': r'const int To = T / 2;.*const long total = \(long\)N \* To \* \(C / 4\);',
               'dc_maxpool1d_2_bwd': r'const int Tp = \(T \+ 1\) / 2;.*const long total = \(long\)N \* Tp \* \(C / 4\);',
               'dc_conv1d_k5_c1_fwd': r'const long total = \(long\)N \* T \* \(Cout / 4\);'}
        assert re.search(per.get(entry, r'const long total = \(long\)N \* T \* \(C / 4\);'), body, flags=re.S), entry
    assert sorted(n for n, _ in users) == sorted(seen)
    # each kernel is the grid-stride loop the trip helpers model
    for kernel, fname in set(c1.LAUNCHES.values()):
        m = re.search(r'void %s\(.*?^}' % kernel, _read(fname), flags=re.M | re.S)
        assert m and ('for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {'
                      in m.group(0)), kernel
        assert 'const int cg = (int)(i % C4);' in m.group(0) and re.search(r'const long s = i / C4;', m.group(0)), kernel


def test_trip_helpers_and_decompositions():
    assert c1.trips(1) == (1, 0) and c1.trips(256) == (1, 1) and c1.trips(c1.CAP_ITEMS) == (1, 1)
    assert c1.trips(c1.CAP_ITEMS + 1) == (2, 1) and c1.trips(2 * c1.CAP_ITEMS + 1) == (3, 2)
    assert c1.trip_of(c1.CAP_ITEMS - 1, c1.CAP_ITEMS + 1) == 0 and c1.trip_of(c1.CAP_ITEMS, c1.CAP_ITEMS + 1) == 1
    assert c1.trip_of(700, 1000) == 0                                     # an uncapped grid: one trip
    assert (c1.rows('dc_maxpool1d_2_fwd', 7), c1.rows('dc_maxpool1d_2_bwd', 7), c1.rows('dc_upsample1d_2x_fwd', 7)) == (3, 4, 7)
    # the kernels' own arithmetic, spelled out once per kernel
    assert c1.decompose('dc_conv1d_k5_c1_fwd', (2 * 7 + 5) * 3 + 1, 3, 7, 12) == (2, 5, 1)
    assert c1.decompose('dc_maxpool1d_2_fwd', (2 * 3 + 2) * 3 + 1, 3, 7, 12) == (2, 2, 1)
    assert c1.decompose('dc_maxpool1d_2_bwd', (2 * 4 + 3) * 3 + 2, 3, 7, 12) == (2, 3, 2)
    assert c1.decompose('dc_upsample1d_2x_drop_bwd', (1 * 7 + 6) * 3, 3, 7, 12) == (1, 6, 0)
    rs = np.random.RandomState(0)
    for entry in c1.LAUNCHES:
        N, T, C = 3, 7, 12
        for i in rs.randint(0, c1.total(entry, N, T, C), 20):
            n, t, cg = c1.decompose(entry, int(i), N, T, C)
            assert c1.item_of(entry, n, t, 4 * cg + 3, N, T, C) == i


def test_first_mismatch_names_the_item_and_its_trip():
    N, T, C = 3, 233017, 12
    bad = np.zeros((N, T, C), bool)
    assert c1.first_mismatch('dc_conv1d_k5_c1_fwd', bad, N, T, C) is None
    bad[2, T - 1, 9] = bad[2, T - 1, 11] = True
    msg = c1.first_mismatch('dc_conv1d_k5_c1_fwd', bad, N, T, C)
    assert 'flat item 2097152 = (n 2, t 233016, quad 2)' in msg and 'trip 2 of 2' in msg and '2 wrong elements' in msg
    # two output samples per item: the up-sampling forward; quad 1 of the SECOND output sample comes before quad 2 of the first
    bad = np.zeros((2, 10, 12), bool)
    bad[1, 6, 8] = bad[1, 7, 4] = True
    assert 'flat item %d = (n 1, t 3, quad 1)' % ((5 + 3) * 3 + 1) in c1.first_mismatch('dc_upsample1d_2x_fwd', bad, 2, 5, 12)
    # the single last sample of an odd trace under the pooling backward
    bad = np.zeros((2, 7, 8), bool)
    bad[1, 6, 5] = True
    assert 'flat item %d = (n 1, t 3, quad 1)' % ((4 + 3) * 2 + 1) in c1.first_mismatch('dc_maxpool1d_2_bwd', bad, 2, 7, 8)


@pytest.mark.parametrize('entry', sorted(c1.LAUNCHES))
def test_every_case_lands_in_its_regime(entry):
    cases = c1.CASES[entry]
    assert {r for r, _, _, _ in cases} >= {'cap+1', 'third'}
    quad_kept = set()
    for regime, N, T, C in cases:
        items, C4 = c1.total(entry, N, T, C), C // 4
        assert c1.blocks(items) == c1.CAP_BLOCKS
        quad_kept.add(c1.CAP_ITEMS % C4 == 0)
        if regime == 'cap+1':
            assert items == c1.CAP_ITEMS + 1 and c1.trips(items) == (2, 1)
            # the one second-trip item: quad 2 of the last row of the last trace
            n, t, cg = c1.decompose(entry, c1.CAP_ITEMS, N, T, C)
            assert (n, t, cg) == (N - 1, c1.rows(entry, T) - 1, 2) and C4 == 3
            if entry == 'dc_maxpool1d_2_bwd':
                assert T % 2 == 1 and 2 * t + 1 == T                      # the single sample: skip gradient only
            if entry == 'dc_maxpool1d_2_fwd':
                assert T % 2 == 1 and 2 * t + 2 == T - 1                  # the dropped last sample lies behind its pair
        elif regime == 'third':
            assert 2 * c1.CAP_ITEMS < items < 2 * c1.CAP_ITEMS + c1.CAP_ITEMS / 100 and c1.trips(items) == (3, 2)
        else:
            assert regime == 'short' and entry == 'dc_conv1d_k5_c1_fwd' and T < 5 and c1.trips(items) == (2, 1)
            first = c1.decompose(entry, c1.CAP_ITEMS, N, T, C)
            assert first[0] < N - 1000 and first[1] != 0                  # the second trip begins inside a trace, many follow
        for name, nbytes in c1.buffers(entry, N, T, C).items():
            assert 0 < nbytes < c1.MAX_BUFFER_BYTES, (entry, regime, name, nbytes)
    assert quad_kept == {True, False}                                     # C4 = 3 or 6 rotates the quad per trip, C4 = 4 or 8 keeps it
    if entry == 'dc_conv1d_k5_c1_fwd':
        assert c1.total(entry, *cases[1][1:]) - 2 * c1.CAP_ITEMS == 5732  # the ragged third trip
    assert c1.PAD == 4 and c1.total(entry, *c1.RNG_SMALL) < c1.THREADS    # the small RNG pin: one workgroup


def test_the_engine_case_reaches_what_it_claims():
    e = c1.ENGINE
    capped, grids, head = c1.engine_launches(e['B'], e['T'], e['nfb'])
    items = [(entry, c1.total(entry, N, T, C)) for entry, N, T, C in capped]
    assert [n for en, n in items if en == 'dc_conv1d_k5_c1_fwd'] == [4509696]
    assert [n for en, n in items if en == 'dc_upsample1d_2x_fwd'] == [4509696] * 4
    assert [n for en, n in items if en == 'dc_maxpool1d_2_fwd'] == [2254848] * 4
    assert c1.trips(4509696) == (3, 2) and c1.trips(2254848) == (2, 1)
    for entry, N, T, C in capped:
        if entry == 'dc_maxpool1d_2_fwd':                                 # the second trip begins with trace 1024 on every level
            assert c1.decompose(entry, c1.CAP_ITEMS, N, T, C) == (1024, 0, 0)
    assert c1.decompose('dc_conv1d_k5_c1_fwd', c1.CAP_ITEMS, e['B'], e['T'], e['nfb']) == (512, 0, 0)
    assert len(grids) == 17 and max(grids) == 35232 and min(grids) == 2202 and min(grids) % 8 and head == 24222
    # a batch of `sub` traces stays on the first trip of every capped launch, so it is an independent witness
    sub_capped, sub_grids, _ = c1.engine_launches(e['sub'], e['T'], e['nfb'])
    assert all(c1.trips(c1.total(*c)) == (1, 1) for c in sub_capped) and len(sub_capped) == 9
    assert max(c1.total(*c) for c in sub_capped) == 1048576
    assert e['B'] % e['sub'] and set(e['oracle_traces']) == {0, 1, 1023, 1024, e['B'] - 2, e['B'] - 1}
    # 1.1 GB of engine buffers (deep_calcium_amd/unet1d.py _buffers: a, b, pool / 2, four concat buffers of 3)
    per = e['B'] * e['T'] * e['nfb'] * 4
    assert 1.0e9 < per * (2 + 0.5 + 12) < 1.1e9
