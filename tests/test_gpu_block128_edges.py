"""Blocks of 65..128 pivots per sweep at the edges tests/test_gpu_block128.py leaves out: a workgroup of k_sweep128_mfma that
takes more than one chunk (more chunks than workgroup slots), its four instantiations <NT, OOP>, tile counts with one range,
two ranges and an empty range, LPs that end at every position of a block (optimal and unbounded), block lengths 65..127 and
the 64 | 65 boundary of valid pivots, the loop-form options, and the tracked slot.  Every case runs in both arithmetic modes
and compares status, pivot count and every bit of A, b, c, v and perm with the oracle of its mode after every call.  A test
asserts the path it claims: where the last sweep of a call took 65..128 decisions, the kernel, the block, the non-temporal
flag and the CUs of the sweep as lpx_state_info reports them; a condition on the input (the LP is still running, the LP is
unbounded, there are more chunks than workgroups) is asserted too."""
import numpy as np
import pytest

from tests.test_gpu_block128 import _loops_vs_oracle
from tests.test_gpu_parity import assert_state_bits_equal, dense_lp

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


@pytest.fixture(scope="module")
def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sweep_kernel(arith, m, n):
    """The sweep of a block of 65..128 decisions: one pass on the matrix cores in the fused arithmetic over whole 512-column
    strips of 16-row tiles, otherwise four passes of the generic kernel."""
    return "k_sweep128_mfma" if (arith == "fused" and m % 16 == 0 and n % 512 == 0) else "k_update_multi"


def _assert_path(st, arith, shape, device_cus, block=128, nt=0, sweep_cus=None):
    """Behind a call whose last sweep took 65..128 decisions.  sweep_cus: None = what the loop form leaves the sweep (the
    whole device in the serial forms and without CU masks, the device less the decisions' CUs on the masked stream)."""
    info = st.info()
    m, n = shape
    assert info["sweep_kernel_name"] == _sweep_kernel(arith, m, n), info
    assert info["block"] == block, info
    assert info["nontemporal"] == nt, info
    if sweep_cus is None:
        sweep_cus = device_cus
        if info["overlapped"] and info["chain_stream_masked"]:
            sweep_cus -= info["chain_resident_max"] // info["chain_blocks_per_cu"]
    assert info["sweep_cus"] == sweep_cus, info
    return info


def _chunks(m, n):
    """Chunks (64-column sub-strip, row range) of k_sweep128_mfma."""
    return (n // 64) * min(3, m // 16)


# ------------------------------------------------------------------------------------ A: more chunks than workgroups
@pytest.mark.parametrize("shape", [(1024, 2048), (64, 1024)])
def test_a_workgroup_takes_several_chunks_out_of_place(lps, oracle, arith, device_cus, shape):
    """sweep_cus = 8 leaves the masked sweep stream 8 CUs, so 16 workgroups of k_sweep128_mfma against 96 chunks (1024 x 2048)
    and 48 chunks, a third of them empty (64 x 1024: four tiles in ranges of 2, 2 and 0): every workgroup takes several
    chunks, reloads its B operands between sub-strips, and passes the barrier between chunks.  Budgets 255 (two full blocks
    out of place), 300, 255 again on whatever buffer the second call left."""
    m, n = shape
    A, b, c = dense_lp(m, n, seed=13 * m + n)
    seen = []

    def after(k, st):
        if k in (0, 2):   # 256 decisions: the call's last block took 128
            info = _assert_path(st, arith, shape, device_cus, sweep_cus=8)
            assert info["overlapped"] == 1 and info["chain_stream_masked"] == 1, info
            assert 2 * info["sweep_cus"] < _chunks(m, n), info
            seen.append(k)

    status = _loops_vs_oracle(lps, oracle, A, b, c, (255, 300, 255), "sweep_cus 8 on %s" % (shape,), after=after,
                              options={"sweep_cus": 8})
    assert status == 9 and seen == [0, 2]


def test_a_workgroup_takes_several_chunks_in_place(lps, oracle, arith, device_cus):
    """256 x 12288 in the serial loop (overlap = 0): 576 chunks against two workgroups on each CU of the whole device, in
    place, several blocks in a call."""
    m, n = 256, 12288
    A, b, c = dense_lp(m, n, seed=13 * m + n)
    seen = []

    def after(k, st):
        if k == 0:
            info = _assert_path(st, arith, (m, n), device_cus)
            assert info["overlapped"] == 0, info
            assert 2 * info["sweep_cus"] < _chunks(m, n), info
            seen.append(k)

    status = _loops_vs_oracle(lps, oracle, A, b, c, (255, 300), "256 x 12288 in place", after=after, options={"overlap": 0})
    assert status == 9 and seen == [0]


# ------------------------------------------------------------------------------------ B: tile-count edges
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("shape", [(16, 512), (32, 512), (64, 512), (80, 1024)])
def test_tile_count_edges(lps, oracle, arith, device_cus, shape, overlap):
    """One tile (one range), two tiles (two ranges of one), four tiles (ranges of 2, 2 and 0: chunks without a tile) and
    five tiles (2, 2, 1), out of place and in place.  Budget 127 is one full block; 255 two; -1 runs the LP through several
    full blocks to its optimum (the one-tile LP is through within the second call)."""
    m, n = shape
    A, b, c = dense_lp(m, n, seed=3)
    seen = []

    def after(k, st):   # (while the LP is running: the call's last block took 128 decisions)
        info = _assert_path(st, arith, shape, device_cus)
        assert info["overlapped"] == (1 if overlap and k == 1 else 0), info   # (a budget that fits one block runs serially)
        seen.append(k)

    status = _loops_vs_oracle(lps, oracle, A, b, c, (127, 255, -1), "tiles of %s, overlap %d" % (shape, overlap), after=after,
                              options={"overlap": overlap})
    assert status == 0 and seen == ([0] if m == 16 else [0, 1])


# ------------------------------------------------------------------------------------ C: the four instantiations
@pytest.mark.parametrize("overlap,nt", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_blocks_of_128_in_place_and_out_of_place_with_and_without_nt(lps, oracle, arith, device_cus, overlap, nt):
    """k_sweep128_mfma<NT, OOP>: in place over several blocks in the serial loop, out of place beside the decisions, with and
    without the non-temporal hints (the counterpart of test_blocks_of_64_in_place_and_out_of_place_with_and_without_nt).
    Budgets 255 (blocks of 128 and 128), 300 (128, 128, 45), 100 (one block of 101 decisions, in place in either loop)."""
    shape = (1024, 2048)
    A, b, c = dense_lp(*shape, seed=13 * 1024 + 2048)
    seen = []

    def after(k, st):
        if k in (0, 2):
            info = _assert_path(st, arith, shape, device_cus, nt=nt)
            assert info["overlapped"] == (overlap if k == 0 else 0), info
            seen.append(k)

    status = _loops_vs_oracle(lps, oracle, A, b, c, (255, 300, 100), "overlap %d nt %d" % (overlap, nt), after=after,
                              options={"overlap": overlap, "nt": nt})
    assert status == 9 and seen == [0, 2]


# ------------------------------------------------------------------------------------ D: block lengths, the 64 | 65 boundary
D_SHAPES = [((256, 512), 21), ((250, 700), 13 * 250 + 700)]   # whole strips; ragged


@pytest.mark.parametrize("block", [65, 96, 127])
@pytest.mark.parametrize("shape,seed", D_SHAPES)
def test_block_lengths_65_to_127(lps, oracle, arith, device_cus, shape, seed, block):
    """lpx_state_set_block takes 65..127 and the 128-slot kernels run them partly filled.  Budgets block - 1 (one full
    block), 2 block + 5 (two and a tail of six), 3 block (three and a decision that only reports the limit)."""
    A, b, c = dense_lp(*shape, seed=seed)
    seen = []

    def after(k, st):
        if k in (0, 2):
            _assert_path(st, arith, shape, device_cus, block=block)
            seen.append(k)

    status = _loops_vs_oracle(lps, oracle, A, b, c, (block - 1, 2 * block + 5, 3 * block), "block %d on %s" % (block, shape),
                              after=after, block=block)
    assert status == 9 and seen == [0, 2]


@pytest.mark.parametrize("shape,seed", D_SHAPES)
def test_64_and_65_valid_pivots_in_a_block_of_128(lps, oracle, arith, device_cus, shape, seed):
    """Budgets 64, 65, 192, 193: the calls' last blocks take 65, 66, 65 and 66 decisions, of which 64, 65, 64 and 65 are
    valid pivots — either side of the word boundary of the pivot count's two ballots."""
    A, b, c = dense_lp(*shape, seed=seed)
    seen = []

    def after(k, st):
        _assert_path(st, arith, shape, device_cus)
        seen.append(k)

    status = _loops_vs_oracle(lps, oracle, A, b, c, (64, 65, 192, 193), "64 | 65 on %s" % (shape,), after=after)
    assert status == 9 and seen == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------ E: endings at every position of a block
def _ending_lp(unbounded):
    A, b, c = dense_lp(64, 512, seed=3)
    if unbounded:
        A[:, -1] = -A[:, -1]
    return A, b, c


@pytest.fixture(scope="module")
def endings(oracle):
    """The oracle's side of the ending tests, computed once per LP and r and shared by the two loop forms: the total pivot
    count P and the final status, and per r the results and states behind a budget of P - r and behind the run to the end."""
    cache = {}

    def get(unbounded):
        if unbounded not in cache:
            A, b, c = _ending_lp(unbounded)
            ref = oracle.State(A, b, c, kind=oracle.FP64)
            end = ref.simplex_loop(max_pivots=-1)
            ref.close()
            cache[unbounded] = {"P": end["pivots"], "status": end["status"], "r": {}}
        return cache[unbounded]

    def at(unbounded, r):
        ent = get(unbounded)
        if r not in ent["r"]:
            A, b, c = _ending_lp(unbounded)
            ref = oracle.State(A, b, c, kind=oracle.FP64)
            first = ref.simplex_loop(max_pivots=ent["P"] - r)
            state1 = ref.read()
            last = ref.simplex_loop(max_pivots=-1)
            state2 = ref.read()
            ref.close()
            ent["r"][r] = ((first["status"], first["pivots"]), state1, (last["status"], last["pivots"]), state2)
        return ent["r"][r]

    return get, at


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("unbounded", [False, True], ids=["optimal", "unbounded"])
def test_lp_ends_at_every_position_of_a_block(lps, oracle, arith, endings, unbounded, overlap):
    """A first call of P - r pivots leaves the LP running, a second one ends it r decisions into its first block of 128:
    r = 1, 63, 64, 65 (the word boundary of the pivot count's two ballots, of the fix-up's hit words and of the decision
    kernel's four-word ballots), 127, 128 (the first decision of the second block: a block with no valid pivot — in place
    the sweep returns, out of place it must carry the tableau over and the buffers must still swap right) and 129.  r = 0: a
    budget of exactly P does not leave the LP running — the decision behind the last pivot finds the ending before it would
    report the limit, in the oracle as on the device — so there the first call ends the LP wherever in a block P falls, and
    the second call's first decision finds the ended LP: a first block with no valid pivot.  One LP ends OPTIMAL, the other —
    its last column negated — UNBOUNDED.  A further call finds the ended LP as it is: same status, no pivot, no bit changed."""
    get, at = endings
    P, final = get(unbounded)["P"], get(unbounded)["status"]
    assert P > 257 and final == (1 if unbounded else 0), (P, final)
    A, b, c = _ending_lp(unbounded)
    for r in (0, 1, 63, 64, 65, 127, 128, 129):
        what = "%s, overlap %d, r %d" % ("unbounded" if unbounded else "optimal", overlap, r)
        want1, state1, want2, state2 = at(unbounded, r)
        assert want1 == ((9, P - r) if r else (final, P)) and want2 == (final, r), what
        st = lps.LPState(A, b, c, block=128, options={"overlap": overlap})
        status, pivots, _ = st.simplex_loop(max_pivots=P - r)
        assert (status, pivots) == want1, what
        assert_state_bits_equal(st.read(), state1, what + ", call 1")
        status, pivots, _ = st.simplex_loop(max_pivots=-1)
        assert (status, pivots) == want2, what
        assert_state_bits_equal(st.read(), state2, what + ", call 2")
        info = st.info()
        assert info["block"] == 128 and info["overlapped"] == overlap, info
        status, pivots, _ = st.simplex_loop(max_pivots=-1)
        assert (status, pivots) == (final, 0), what
        assert_state_bits_equal(st.read(), state2, what + ", call 3")
        st.close()


# ------------------------------------------------------------------------------------ F: loop forms at 128
@pytest.mark.parametrize("shape", [(1024, 1024), (400, 1300)])
@pytest.mark.parametrize("knobs", [
    {"overlap": 0},                              # the decisions, then the in-place sweep, one after the other
    {"overlap_serial": 1},                       # out-of-place sweeps without concurrency
    {"overlap_mask": 0},                         # decisions beside the sweep without CU masks
    {"chain_wgs": 1}, {"chain_wgs": 3},          # four and more rows, eight and more columns per thread of k_block_decide128
    {"chain_wgs": 7, "overlap": 0},
    {"chain_fences": 3},                         # release + acquire at every grid barrier
    {"sweep_rows": 64},
    {"chain": 0},                                # three launches per decision: holds 32 pending pivots, the block is clamped
], ids=lambda k: ",".join("%s=%s" % kv for kv in sorted(k.items())))
def test_loop_forms_with_blocks_of_128(lps, oracle, arith, device_cus, knobs, shape):
    """The loop-form options of test_blocked_loop_forms_are_bit_identical with block = 128, on whole strips and on a ragged
    shape.  Budgets 127 (one block), 2 x 128 + 3, 5 x 128 (five blocks and a decision that only reports the limit), 1.
    chain = 0 clamps the block to 32 (choose_block): asserted, and parity all the same."""
    m, n = shape
    A, b, c = dense_lp(m, n, seed=7 * m + n)
    clamped = knobs.get("chain", 1) == 0
    seen = []

    def after(k, st):
        for key, v in knobs.items():
            assert st.get_option(key) == v
        if k in (0, 2):
            if clamped:
                assert st.info()["block"] == 32, st.info()
            else:
                info = _assert_path(st, arith, shape, device_cus)
                if "chain_wgs" in knobs:   # (the launcher takes no more workgroups than one row / column per thread asks for)
                    assert info["chain_wgs_requested"] == knobs["chain_wgs"] and 1 <= info["chain_wgs"] <= knobs["chain_wgs"], info
                if knobs.get("overlap_mask", 1) == 0 and k == 2:
                    assert info["overlapped"] == 1 and info["chain_stream_masked"] == 0, info
            seen.append(k)

    status = _loops_vs_oracle(lps, oracle, A, b, c, (127, 2 * 128 + 3, 5 * 128, 1), "%s on %s" % (knobs, shape), after=after,
                              want_block=32 if clamped else None, options=knobs)
    assert status == 9 and seen == [0, 2]


# ------------------------------------------------------------------------------------ G: the tracked slot
def _slot_of(perm, variable):
    hits = np.flatnonzero(np.asarray(perm) == variable)
    assert hits.size == 1, (variable, hits)
    return int(hits[0])


def test_tracked_slot_is_where_perm_has_the_variable(lps, oracle):
    """The reading the next test relies on, on the phase-1 case of test_blocked_pivoting_degenerate_unbounded_and_tracking
    (block = 2): the tracked slot goes through the same exchanges of slots e and n + l as perm, so behind a call it is the
    slot at which perm holds the variable that sat in the slot handed in."""
    A = [[1, 0, -1], [-1, 0, -1], [0, 1, -1], [0, -1, -1]]
    b, c = [10, -2, 10, -2], [0, 0, -1]
    aux = lps.LPState(A, b, c, block=2)
    ref = oracle.State(np.array(A, dtype=np.float64), b, c, kind=oracle.FP64)
    aux.pivot(2, 1)
    ref.pivot(2, 1)
    variable = int(aux.perm[1 + 3])
    assert variable == 2 and int(ref.read()[4][1 + 3]) == 2   # x0 left slot 2 for the slot of row 1
    status, pivots, x0 = aux.simplex_loop(track_slot=1 + 3)
    want = ref.simplex_loop()
    assert (status, pivots) == (want["status"], want["pivots"]) and status == 0
    assert_state_bits_equal(aux.read(), ref.read(), "phase 1, block 2")
    assert x0 == _slot_of(ref.read()[4], variable) == 1
    aux.close()
    ref.close()


@pytest.mark.parametrize("where", ["first", "last", "basic"])
def test_tracked_slot_with_blocks_of_128(lps, oracle, where):
    """track_slot through 128-slot decisions: 300 pivots (blocks of 128, 128 and 45), then the rest of the LP from the slot
    the first call returned.  After either call the returned slot is where the oracle's perm holds the variable."""
    m, n = 64, 512
    A, b, c = dense_lp(m, n, seed=3)
    t = {"first": 0, "last": n - 1, "basic": n + m // 2}[where]
    st = lps.LPState(A, b, c, block=128)
    ref = oracle.State(A, b, c, kind=oracle.FP64)
    assert int(ref.read()[4][t]) == t   # a fresh handle: variable t sits in slot t
    slot = t
    for k, budget in enumerate((300, -1)):
        status, pivots, got = st.simplex_loop(max_pivots=budget, track_slot=slot)
        want = ref.simplex_loop(max_pivots=budget)
        assert (status, pivots) == (want["status"], want["pivots"]) == ((9, 300) if k == 0 else (0, pivots)), (where, budget)
        assert_state_bits_equal(st.read(), ref.read(), "tracking %s, call %d" % (where, k))
        assert got == _slot_of(ref.read()[4], t), (where, budget, got)
        slot = got
    assert st.info()["block"] == 128, st.info()
    st.close()
    ref.close()
