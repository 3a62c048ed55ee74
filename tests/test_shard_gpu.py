"""Row sharding on the device (gbrs_shard_plan / _index / _gather, gbrs_amd/csrc/em_shard.inc) against
gbrs_amd.dist.shard_rows: the same bounds, column pointers, row ids, values and counts, bit for bit."""
import numpy as np
import pytest

from conftest import em_case_inputs, em_case_values, golden_files, load_golden

pytestmark = pytest.mark.gpu


def _bounds_numpy(indices, R, world):
    per_row = np.zeros(R, dtype=np.int64)
    for ix in indices:
        per_row += np.bincount(ix, minlength=R)
    cum = np.concatenate(([0], np.cumsum(per_row)))
    b = [int(np.searchsorted(cum, cum[-1] * k / world, side="left")) for k in range(world + 1)]
    b[0], b[-1] = 0, R
    return b


def _straddling_numpy(ip, ix, l_split, n_rows):
    in_a, in_b = np.zeros(n_rows, bool), np.zeros(n_rows, bool)
    for p, x in zip(ip, ix):
        cut = int(p[l_split])
        in_a[x[:cut].astype(np.int64)] = True
        in_b[x[cut:].astype(np.int64)] = True
    return int((in_a & in_b).sum())


def _device(torch, arrays, dtype=None):
    return [torch.from_numpy(np.ascontiguousarray(a).view(dtype) if dtype else np.ascontiguousarray(a)).to("cuda:0")
            for a in arrays]


def _check_against_shard_rows(R, L, H, indptr, indices, count, values, worlds, l_split=None):
    import torch
    from gbrs_amd.dist import shard_rows
    from gbrs_amd.sharded import shard_block, shard_plan
    ip = _device(torch, indptr, np.int32)
    ix = _device(torch, indices, np.int32)
    vals = None if values is None else _device(torch, values)
    torch.cuda.synchronize()
    ls = l_split if l_split is not None else L // 2
    for world in worlds:
        bounds = shard_plan(R, L, H, ip, ix, world, 0)
        assert bounds == _bounds_numpy(indices, R, world), world
        for rank in range(world):
            r0, r1, e_ip, e_ix, e_cnt = shard_rows(indptr, indices, count, R, rank, world)
            assert (bounds[rank], bounds[rank + 1]) == (r0, r1)
            g_ip, g_ix, g_v, straddling = shard_block(torch, R, L, H, ip, ix, vals, r0, r1, ls, 0)
            for h in range(H):
                np.testing.assert_array_equal(g_ip[h].cpu().numpy().view(np.uint32), e_ip[h])
                np.testing.assert_array_equal(g_ix[h].cpu().numpy().view(np.uint32), e_ix[h])
                if values is not None:
                    keep = (indices[h] >= r0) & (indices[h] < r1)
                    np.testing.assert_array_equal(g_v[h].cpu().numpy(), values[h][keep])
            assert straddling == _straddling_numpy(e_ip, e_ix, ls, r1 - r0)
            if count is not None:
                np.testing.assert_array_equal(count[r0:r1], e_cnt)


@pytest.mark.parametrize("path", golden_files("em"), ids=lambda p: p.split("/")[-1][:-4])
def test_device_shards_equal_shard_rows_on_goldens(path):
    g = load_golden(path)
    R, L, H, indptr, indices, count, eff_len, groups, gtmask = em_case_inputs(g)
    _check_against_shard_rows(R, L, H, indptr, indices, count, em_case_values(g), (1, 2, 3, 8))


def _random_csc(R, L, H, seed, per_row_max=6, empty_frac=0.2):
    """Random rows, a fifth of them empty."""
    rng = np.random.default_rng(seed)
    nl = rng.integers(1, per_row_max + 1, size=R)
    nl[rng.random(R) < empty_frac] = 0
    rows = np.repeat(np.arange(R, dtype=np.int64), nl)
    loci = np.concatenate([rng.choice(L, size=k, replace=False) for k in nl if k] or [np.zeros(0, np.int64)])
    masks = rng.integers(1, 1 << H, size=len(rows), dtype=np.int64)
    indptr, indices = [], []
    for h in range(H):
        sel = (masks >> h) & 1 == 1
        order = np.lexsort((rng.random(int(sel.sum())), loci[sel]))     # rows in no particular order inside a column
        indices.append(rows[sel][order].astype(np.uint32))
        indptr.append(np.searchsorted(loci[sel][order], np.arange(L + 1)).astype(np.uint32))
    values = [rng.random(len(ix)) for ix in indices]
    count = rng.integers(1, 5, size=R).astype(np.float64)
    return indptr, indices, count, values


@pytest.mark.parametrize("H", [1, 16])
def test_device_shards_random_with_empty_rows(H):
    R, L = 5000, 300
    indptr, indices, count, values = _random_csc(R, L, H, seed=H)
    _check_against_shard_rows(R, L, H, indptr, indices, count, values, (1, 2, 3, 8, 13), l_split=L // 3)


def test_device_shards_one_column_of_over_a_million_entries():
    R, L = 1_500_000, 40
    rng = np.random.default_rng(5)
    heavy = rng.choice(R, size=1_200_000, replace=False)
    other = np.unique(rng.integers(0, R, size=600_000) * L + rng.integers(0, L, size=600_000))
    other = other[other % L != 17]
    rows = np.concatenate([heavy, other // L])
    loci = np.concatenate([np.full(len(heavy), 17), other % L])
    order = np.lexsort((rng.random(len(rows)), loci))            # rows in no particular order inside a column
    indices = [rows[order].astype(np.uint32)]
    indptr = [np.searchsorted(loci[order], np.arange(L + 1)).astype(np.uint32)]
    assert int(np.diff(indptr[0].astype(np.int64)).max()) > 1_000_000
    values = [rng.random(len(indices[0]))]
    count = rng.integers(1, 5, size=R).astype(np.float64)
    _check_against_shard_rows(R, L, 1, indptr, indices, count, values, (2, 8), l_split=17)


def test_device_shards_a_block_of_one_row():
    """Row 0 holds most entries: a world of 4 gives it a block of its own (and leaves two blocks empty)."""
    R, L, H = 200, 1000, 1
    rng = np.random.default_rng(3)
    rows = np.concatenate([np.full(900, 0), rng.integers(0, R, size=150)])
    loci = np.concatenate([np.arange(900), rng.integers(900, L, size=150)])
    key = np.unique(loci.astype(np.int64) * R + rows)
    loci, rows = key // R, key % R
    indices = [rows.astype(np.uint32)]
    indptr = [np.searchsorted(loci, np.arange(L + 1)).astype(np.uint32)]
    bounds = _bounds_numpy(indices, R, 4)
    assert 1 in np.diff(bounds)
    _check_against_shard_rows(R, L, H, indptr, indices, None, None, (4,))


def test_out_of_range_row_id_is_an_error():
    import torch
    from gbrs_amd import _lib
    from gbrs_amd.sharded import shard_block, shard_plan
    R, L = 100, 10
    ix_h = np.arange(50, dtype=np.uint32)
    ix_h[37] = R + 5
    ip_h = np.linspace(0, 50, L + 1).astype(np.uint32)
    ip, ix = _device(torch, [ip_h], np.int32), _device(torch, [ix_h], np.int32)
    torch.cuda.synchronize()
    with pytest.raises(_lib.GbrsHipError) as e:
        shard_plan(R, L, 1, ip, ix, 2, 0)
    assert e.value.status == _lib.GBRS_ERR_INVALID
    with pytest.raises(_lib.GbrsHipError) as e:
        shard_block(torch, R, L, 1, ip, ix, None, 0, 50, 0, 0)
    assert e.value.status == _lib.GBRS_ERR_INVALID
    bad_ip = ip_h.copy()
    bad_ip[3] = 60                              # past the end of indices: refused before the scan is read there
    with pytest.raises(_lib.GbrsHipError) as e:
        shard_plan(R, L, 1, _device(torch, [bad_ip], np.int32), ix, 2, 0)
    assert e.value.status == _lib.GBRS_ERR_INVALID
