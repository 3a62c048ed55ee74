"""`gbrs interpolate` and the dosage product of `gbrs export` on the device at their edges (needs an MI355X).

Interpolation is compared bit for bit with the CPU oracle, which is itself bit-equal to scipy's interp1d
(tests/test_small_ops_cpu.py): the kernel does one subtraction and one division for the slope, then one multiplication
and one addition, in scipy's order, and the library is built without FMA contraction, so every operation rounds as
numpy's does.  The dosage of one-hot rows is exact; that of random rows is within 2 S 2^-53 of the exactly rounded sum."""
import numpy as np
import pytest

import small_ops_cases as cases

pytestmark = pytest.mark.gpu

INTERP = [(name, S) for name in cases.interp_positions() for S in cases.STATE_COUNTS
          if S in (3, 136) or name in ("on_knots", "one_gene")]


@pytest.mark.parametrize("name,S", INTERP)
def test_interpolate_equals_the_oracle(name, S):
    from gbrs_amd.postproc import interpolate_arrays
    from oracle import postproc_oracle
    x_gene, gamma, x_grid = cases.interp_case(name, S)
    expected = postproc_oracle.interpolate(x_gene, gamma, x_grid)
    out = interpolate_arrays(x_gene, gamma, x_grid)
    assert out.shape == (S, len(x_grid))
    np.testing.assert_array_equal(out, expected)


def test_interpolate_edge_values():
    """A query on a position that several genes share takes the value of the first of them (the segment that ends
    there); queries before the first or after the last gene take the first or the last column."""
    from gbrs_amd.postproc import interpolate_arrays
    err = 4 * 2.0 ** -53          # four roundings (subtract, divide, multiply, add) of values within [-1, 1]
    for name in ("two_at_one_position", "three_at_one_position"):
        x_gene, gamma, x_grid = cases.interp_case(name, 36)
        out = interpolate_arrays(x_gene, gamma, x_grid)
        assert x_grid[1] == x_gene[1] == x_gene[2]
        np.testing.assert_allclose(out[:, 1], gamma[:, 1], rtol=0, atol=err)
        assert np.abs(gamma[:, 1] - gamma[:, 2]).max() > 1e-3
    x_gene, gamma, x_grid = cases.interp_case("before_first_gene", 136)
    np.testing.assert_array_equal(interpolate_arrays(x_gene, gamma, x_grid), np.repeat(gamma[:, :1], 3, axis=1))
    x_gene, gamma, x_grid = cases.interp_case("after_last_gene", 136)
    np.testing.assert_array_equal(interpolate_arrays(x_gene, gamma, x_grid), np.repeat(gamma[:, -1:], 3, axis=1))
    x_gene, gamma, x_grid = cases.interp_case("grid_zero", 3)
    np.testing.assert_array_equal(interpolate_arrays(x_gene, gamma, x_grid)[:, 0], gamma[:, 0])


def test_interpolate_wrapper_errors():
    from gbrs_amd.postproc import interpolate_arrays
    x_gene, gamma, x_grid = cases.interp_case("after_last_gene", 3)
    with pytest.raises(ValueError, match="below the interpolation range"):
        interpolate_arrays(x_gene, gamma, np.array([-1e-300, 2.0]))
    with pytest.raises(ValueError, match="above the interpolation range"):
        interpolate_arrays(x_gene, gamma, np.array([9.0, 3.0]))       # the last knot is the last grid point + 1
    np.testing.assert_array_equal(interpolate_arrays(x_gene, gamma, x_grid), np.repeat(gamma[:, -1:], 3, axis=1))


def test_interpolate_raw_errors():
    from gbrs_amd import _lib
    lib = _lib.load()
    x = np.array([0.0, 1.0, 2.0, 4.0])
    y = np.ascontiguousarray(cases.gamma_columns(3, 4, 1))
    grid = np.array([0.5, 3.0])

    def call(n_points, xs, n_grid, q):
        out = np.full((3, 2), -1.0)
        st = lib.gbrs_interpolate(3, n_points, _lib.ptr(xs), _lib.ptr(y), n_grid, _lib.ptr(q), _lib.ptr(out), 0)
        return st, out

    for n_points, xs, n_grid, q, message in (
            (4, x, 2, np.array([-0.5, 3.0]), b"below the interpolation range"),
            (4, x, 2, np.array([0.5, 4.5]), b"above the interpolation range"),
            (4, np.ascontiguousarray(x[::-1]), 2, grid, b"ascending"),
            (1, x, 2, grid, b"bad argument")):
        st, out = call(n_points, xs, n_grid, q)
        assert st == _lib.GBRS_ERR_INVALID and message in lib.gbrs_last_error()
        assert (out == -1.0).all()
    st, out = call(4, x, 0, grid)
    assert st == _lib.GBRS_OK and (out == -1.0).all()                    # n_grid = 0: nothing to do, out untouched
    st, out = call(4, x, 2, grid)
    assert st == _lib.GBRS_OK
    slope = (y[:, [1, 3]] - y[:, [0, 2]]) / np.array([1.0, 2.0])
    np.testing.assert_array_equal(out, slope * np.array([0.5, 1.0]) + y[:, [0, 2]])


def dosage(H, rows):
    from gbrs_amd import _lib
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    out = np.full((rows.shape[0], H), -1.0)
    _lib.check(_lib.load().gbrs_genoprob_dosage(H, rows.shape[0], _lib.ptr(rows), _lib.ptr(out), 0))
    return out


@pytest.mark.parametrize("H", [1, 2, 3, 4, 8, 16])
def test_dosage_one_hot_rows(H):
    """Genotype (a, b), a <= b, a outer: 0.5 to a and 0.5 to b, 1.0 when a = b.  Exact."""
    rows, expected = cases.dosage_one_hot(H)
    np.testing.assert_array_equal(dosage(H, rows), expected)


@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 1000])
@pytest.mark.parametrize("H", [1, 2, 3, 8, 16])
def test_dosage_random_rows(H, n_rows):
    rows, expected = cases.dosage_random(H, n_rows)
    np.testing.assert_allclose(dosage(H, rows), expected, rtol=cases.dosage_rtol(H), atol=0)


def test_dosage_zero_rows_and_arguments():
    from gbrs_amd import _lib
    lib = _lib.load()
    np.testing.assert_array_equal(dosage(8, np.zeros((40, 36))), np.zeros((40, 8)))
    out = np.full((2, 17), -1.0)
    rows = np.zeros((2, 17 * 18 // 2))
    assert lib.gbrs_genoprob_dosage(4, 0, _lib.ptr(rows), _lib.ptr(out), 0) == _lib.GBRS_OK
    assert lib.gbrs_genoprob_dosage(4, 0, None, None, 0) == _lib.GBRS_OK
    for H in (0, 17):
        assert lib.gbrs_genoprob_dosage(H, 2, _lib.ptr(rows), _lib.ptr(out), 0) == _lib.GBRS_ERR_INVALID
    assert (out == -1.0).all()
