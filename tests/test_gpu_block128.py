"""Blocks of 65..128 pivots per sweep, end to end (block = 128): the 128-slot decision kernel k_block_decide128 (256 pending
pivots, up to four windows per ladder), the fix-up over 128 pending pivots, and the sweep — in the fused arithmetic over whole
512-column strips of 16-row tiles ONE pass of k_sweep128_mfma on the matrix cores, otherwise four passes of the generic
kernel over slots 0.., 32.., 64.., 96...  Every case runs in both arithmetic modes and compares bit for bit with the oracle
of its mode; the shapes are the smallest that reach the paths named in the docstrings."""
import numpy as np
import pytest

from tests.test_gpu_parity import _timed_form_vs_oracle, assert_state_bits_equal, dense_lp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lps(arith):
    from tests.conftest import package_in_mode
    pkg = package_in_mode(arith)
    yield pkg
    pkg.set_default_arithmetic("auto")


@pytest.fixture(scope="module")
def oracle(arith):
    from oracle import pyoracle
    from tests.conftest import ArithOracle
    pyoracle.build()
    pyoracle.lib()
    return ArithOracle(pyoracle, arith)


def _loops_vs_oracle(lps, oracle, A, b, c, budgets, what, pricing=None, after=None, block=128, want_block=None, **kw):
    """Resumed loop calls with block = 128 (or `block`) against the oracle: status, pivots and every bit of the state after
    each call.  after(k, st): a look at the handle behind call k, while the LP is still running.  want_block: what
    lpx_state_info.block must say in the end where an option clamps the block."""
    st = lps.LPState(A, b, c, block=block, **dict(kw, **({"pricing": pricing} if pricing else {})))
    ref = oracle.State(A, b, c, kind=oracle.FP64, pricing=1 if pricing == "dantzig" else 0)
    status = None
    for k, budget in enumerate(budgets):
        status, pivots, _ = st.simplex_loop(max_pivots=budget)
        want = ref.simplex_loop(max_pivots=budget, threads=8)
        assert (status, pivots) == (want["status"], want["pivots"]), (what, budget)
        assert_state_bits_equal(st.read(), ref.read(), "%s, call %d, budget %d" % (what, k, budget))
        if after is not None and status == 9:
            after(k, st)
        if status != 9:
            break
    assert st.info()["block"] == (block if want_block is None else want_block), st.info()
    st.close()
    ref.close()
    return status


@pytest.mark.parametrize("shape", [(1024, 2048), (2048, 1536)])
def test_blocks_of_128_on_whole_strips(lps, oracle, arith, shape):
    """m % 16 == 0 and whole 512-column strips: the fused mode sweeps through k_sweep128_mfma, the default arithmetic through
    four generic passes.  Budgets 127 (one block of 127 pivots and the decision that reports the limit), 2 x 128 + 5 (two full
    blocks beside each other's sweeps and a tail of at most 64 valid pivots), 127 again on the swapped buffers, 300 (blocks of
    128, 128 and 45)."""
    m, n = shape
    A, b, c = dense_lp(m, n, seed=13 * m + n)
    name = "k_sweep128_mfma" if arith == "fused" else "k_update_multi"

    def after(k, st):
        if k in (0, 2):   # the call's last (only) sweep took 127 pivots
            assert st.info()["sweep_kernel_name"] == name, st.info()

    _loops_vs_oracle(lps, oracle, A, b, c, (127, 2 * 128 + 5, 127, 300), "128 on %s" % (shape,), after=after)


@pytest.mark.parametrize("shape", [(1000, 2100), (1536, 700)])
def test_blocks_of_128_on_ragged_shapes(lps, oracle, shape):
    """A partial last strip, m no multiple of 16, a pitch below 1024: the generic passes over slots 0.., 32.., 64.., 96.. in
    both modes."""
    m, n = shape
    A, b, c = dense_lp(m, n, seed=13 * m + n)

    def after(k, st):
        if k in (0, 2):
            assert st.info()["sweep_kernel_name"] == "k_update_multi", st.info()

    _loops_vs_oracle(lps, oracle, A, b, c, (127, 2 * 128 + 5, 127, 300), "128 on %s" % (shape,), after=after)


@pytest.mark.parametrize("shape", [(600, 900), (1536, 700), (1024, 2048)])
@pytest.mark.parametrize("pricing", ["dantzig", None])
def test_blocks_of_128_with_long_ladders(lps, oracle, shape, pricing):
    """Dantzig pricing seldom returns to a slot, so a decision's ladder runs through up to 256 pending pivots: all four
    windows of eight chunks, and the boundary value between the two blocks' pivots in each of them.  Both rules, budgets
    that are no multiples of 128 (the counterpart of test_blocks_of_64_with_long_ladders).  The first two shapes are ragged
    and take the generic passes; 1024 x 2048 has whole strips of 16-row tiles: the long ladders in front of k_sweep128_mfma
    in the fused mode.  That LP is still running after all four budgets under either rule."""
    m, n = shape
    A, b, c = dense_lp(m, n, seed=m + 7 * n)
    whole = m % 16 == 0 and n % 512 == 0
    name = "k_sweep128_mfma" if (oracle.mode == "fused" and whole) else "k_update_multi"

    def after(k, st):
        if k in (0, 1):   # the call's last sweep took 73 / 78 decisions (201 = 128 + 73, 334 = 2 x 128 + 78)
            assert st.info()["sweep_kernel_name"] == name, st.info()

    status = _loops_vs_oracle(lps, oracle, A, b, c, (200, 333, 129, 257), "%s on %s" % (pricing, shape), pricing=pricing,
                              after=after)
    if whole:
        assert status == 9


def test_blocks_of_128_with_two_rows_per_thread(lps, oracle):
    """16400 rows: more than the largest decision grid has threads, so a thread takes two rows (the second pass and its own
    reach of the start indices)."""
    m, n = 16400, 512
    A, b, c = dense_lp(m, n, seed=5)
    _loops_vs_oracle(lps, oracle, A, b, c, (200, 150), "16400 x 512")


def test_blocks_of_128_to_the_end_of_the_lp(lps, oracle):
    """max_pivots = -1: the LP ends inside a block; status, pivots and the state equal the oracle's."""
    m, n = 256, 512
    A, b, c = dense_lp(m, n, seed=21)
    status = _loops_vs_oracle(lps, oracle, A, b, c, (-1,), "256 x 512 to the end")
    assert status == 0


def test_blocks_of_128_on_a_degenerate_lp_with_ties(lps, oracle):
    """A 0/1 matrix with small-integer right-hand sides and costs: massive ties in the ratio test and in the entering rule,
    many degenerate pivots."""
    m, n = 512, 1024
    rng = np.random.default_rng(20241)
    A = (rng.random((m, n)) < 0.3).astype(np.float64)
    b = rng.integers(1, 4, m).astype(np.float64)
    c = rng.integers(1, 4, n).astype(np.float64)
    _loops_vs_oracle(lps, oracle, A, b, c, (300, 200), "0/1 matrix 512 x 1024")


@pytest.mark.parametrize("side", [0, 2])
def test_blocks_of_128_with_the_fixup_behind_and_beside_the_sweep(lps, oracle, side):
    """fixup_side 0 (the fix-up behind the sweep, writing the tableau) and 2 (its chains and the sweep's pack kernel beside
    the sweep, their images copied behind it): three full blocks and a tail."""
    info = _timed_form_vs_oracle(lps, oracle, 1024, 2048, (3 * 128 + 7,), options={"block": 128, "fixup_side": side})
    assert info["block"] == 128 and info["overlapped"] == 1, info


def test_block_policy_by_size_and_budget(lps, arith):
    """choose_block through lpx_state_get_block on the smallest whole-strip shape the size threshold admits (4 GiB, created
    from zeros, no loop): 128 in the fused arithmetic, never in the default one; a pitch that is no multiple of 512 keeps 64.
    lpx_state_info.block is what the last loop call took: a small handle with default options after a short budget."""
    m, n = 16384, 32768
    z = np.zeros((m, n))
    st = lps.LPState(z, np.zeros(m), np.zeros(n))
    assert st.block() == (128 if arith == "fused" else 32), (arith, st.block())
    assert st.info()["block"] == st.block()
    st.close()
    st = lps.LPState(z[:, :n - 256], np.zeros(m), np.zeros(n - 256))
    assert st.block() == (64 if arith == "fused" else 32), (arith, st.block())
    st.close()
    del z
    A, b, c = dense_lp(2048, 2048, seed=2)
    st = lps.LPState(A, b, c)
    want = st.block()
    status, pivots, _ = st.simplex_loop(max_pivots=40)
    assert (status, pivots) == (9, 40)
    assert st.info()["block"] == want == 32, st.info()
    st.close()
