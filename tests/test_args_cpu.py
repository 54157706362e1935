"""The argument rules of the Python front end (minigrid_dynamicprogramming_amd/_args.py): every rule's accepted
form and every refusal, without a GPU or the built library.  B = 2, S = 100, horizon / N = 6 as in the other
front-end CPU tests; the expected messages are those ValueIteration and MiniGridVecEnv have always raised."""
import numpy as np
import pytest

from minigrid_dynamicprogramming_amd import _args

B, S, H, A = 2, 100, 6, 7
DTYPE_MSG = r"policy must be an integer array \(int8 action lanes\), got dtype float32"
FIT_MSG = "policy entries do not fit int8 action lanes"


def _lanes(a, T, shape):
    pi, rows = a
    assert pi.dtype == np.int8 and pi.flags.c_contiguous and pi.shape == shape and rows == T
    return pi


# ---------------------------------------------------------------- the three row rules
def test_evaluate_policy_accepts():
    _lanes(_args.evaluate_policy(np.full((B, S), 3, np.int64), B, S), 1, (B, S))
    _lanes(_args.evaluate_policy(np.zeros((H, B, S), np.uint16), B, S, H, rows=True), H, (H, B, S))
    _lanes(_args.evaluate_policy(np.zeros((B, S), np.int8), B, S, H, rows=True), 1, (B, S))
    strided = np.full((B, 2 * S), -1, np.int8)[:, ::2]  # comes back contiguous, the values kept
    assert (_lanes(_args.evaluate_policy(strided, B, S), 1, (B, S)) == -1).all()


def test_evaluate_policy_refuses():
    with pytest.raises(ValueError, match=DTYPE_MSG):
        _args.evaluate_policy(np.zeros((B, S), np.float32), B, S)
    with pytest.raises(ValueError, match=r"policy of shape \(2, 99\) does not match the handle's \(2, 100\)$"):
        _args.evaluate_policy(np.zeros((B, 99), np.int8), B, S)
    # rows are admitted only where asked for, and only on a finite horizon
    for horizon, rows in ((H, False), (0, True)):
        with pytest.raises(ValueError, match=r"policy of shape \(6, 2, 100\) does not match the handle's \(2, 100\)$"):
            _args.evaluate_policy(np.zeros((H, B, S), np.int8), B, S, horizon, rows=rows)
    with pytest.raises(ValueError, match=r"of shape \(5, 2, 100\) does not match the handle's \(2, 100\) or \(6, 2, 100\)$"):
        _args.evaluate_policy(np.zeros((5, B, S), np.int8), B, S, H, rows=True)
    for bad in (300, -129):
        with pytest.raises(ValueError, match=FIT_MSG):
            _args.evaluate_policy(np.full((B, S), bad, np.int32), B, S)


def test_occupancy_policy_accepts_and_refuses():
    _lanes(_args.occupancy_policy(np.zeros((B, S), np.int32), B, S, H), 1, (B, S))
    _lanes(_args.occupancy_policy(np.zeros((H, B, S), np.int64), B, S, H), H, (H, B, S))
    with pytest.raises(ValueError, match=DTYPE_MSG):
        _args.occupancy_policy(np.zeros((B, S), np.float32), B, S, H)
    with pytest.raises(ValueError, match=r"of shape \(5, 2, 100\) does not match \(2, 100\) or \(6, 2, 100\) \(rows T = 5\)"):
        _args.occupancy_policy(np.zeros((5, B, S), np.int8), B, S, H)
    with pytest.raises(ValueError, match=r"of shape \(2, 99\) does not match \(2, 100\) or \(6, 2, 100\) \(rows T = \?\)"):
        _args.occupancy_policy(np.zeros((B, 99), np.int8), B, S, H)
    with pytest.raises(ValueError, match=FIT_MSG):
        _args.occupancy_policy(np.full((H, B, S), 128, np.int16), B, S, H)


def test_rollout_policy_accepts_and_refuses():
    _lanes(_args.rollout_policy(np.zeros((B, S), np.int64), B, S, "xyd"), 1, (B, S))
    _lanes(_args.rollout_policy(np.zeros((3, B, S), np.uint8), B, S, "xyd"), 3, (3, B, S))
    with pytest.raises(ValueError, match=DTYPE_MSG):
        _args.rollout_policy(np.zeros((B, S), np.float32), B, S, "xyd")
    for shape in ((B, 99), (3, B, 99), (0, B, S), (S,)):
        with pytest.raises(ValueError, match=r"is neither \(2, 100\) nor \(T, 2, 100\) of the doorkey model"):
            _args.rollout_policy(np.zeros(shape, np.int8), B, S, "doorkey")
    with pytest.raises(ValueError, match=FIT_MSG):
        _args.rollout_policy(np.full((3, B, S), 300, np.int32), B, S, "xyd")
    with pytest.raises(ValueError, match=r"a time-indexed policy needs T > 1 rows; pass \(B, S\) for a stationary one"):
        _args.rollout_policy(np.zeros((1, B, S), np.int8), B, S, "xyd")


def test_order_of_checks_on_inputs_wrong_in_two_ways():
    """dtype kind, then shape, then the int8 fit; on the vector side the T > 1 rule last."""
    wrong_shape_float = np.zeros((B, 99), np.float32)
    wrong_shape_300 = np.full((B, 99), 300, np.int32)
    for rule in (lambda a: _args.evaluate_policy(a, B, S, H, rows=True), lambda a: _args.occupancy_policy(a, B, S, H),
                 lambda a: _args.rollout_policy(a, B, S, "xyd")):
        with pytest.raises(ValueError, match=DTYPE_MSG):
            rule(wrong_shape_float)
        with pytest.raises(ValueError, match=r"policy of shape \(2, 99\)"):
            rule(wrong_shape_300)
    with pytest.raises(ValueError, match=FIT_MSG):
        _args.rollout_policy(np.full((1, B, S), 300, np.int32), B, S, "xyd")


# ---------------------------------------------------------------- the other ValueIteration rules
def test_max_iters():
    assert _args.max_iters(1) == 1 and _args.max_iters(np.int64(1000)) == 1000
    for bad in (0, -3):
        with pytest.raises(ValueError, match="max_iters must be > 0"):
            _args.max_iters(bad)


def test_evaluate_rows():
    assert _args.evaluate_rows(1, False, 0) == 1 and _args.evaluate_rows(np.int32(H), True, H) == H
    assert _args.evaluate_rows(1, True, H) == 1
    with pytest.raises(ValueError, match=r"policy rows T = 5: 1 or the handle's horizon \(6\)"):
        _args.evaluate_rows(5, False, H)
    with pytest.raises(ValueError, match=r"policy rows T = 6: 1 or the handle's horizon \(0\)"):
        _args.evaluate_rows(6, True, 0)  # the rows first
    with pytest.raises(ValueError, match="values_t needs a finite horizon"):
        _args.evaluate_rows(1, True, 0)


def test_values_t_horizon():
    assert _args.values_t_horizon(False, 0) is None and _args.values_t_horizon(True, H) is None
    with pytest.raises(ValueError, match="values_t needs a finite horizon"):
        _args.values_t_horizon(True, 0)


def test_occupancy_steps():
    assert _args.occupancy_steps(None, H) == H and _args.occupancy_steps(H, H) == H and _args.occupancy_steps(9, 0) == 9
    with pytest.raises(ValueError, match="n_steps = 5 on a finite-horizon handle: None or the horizon 6"):
        _args.occupancy_steps(5, H)
    with pytest.raises(ValueError, match="n_steps is required on a horizon-0 handle"):
        _args.occupancy_steps(None, 0)


def test_occupancy_start():
    idx, mu0 = _args.occupancy_start(np.array([5, 2 ** 40]), B, S, np.float32)
    assert mu0 is None and idx.dtype == np.int32 and idx.flags.c_contiguous and idx.tolist() == [5, 2 ** 31 - 1]
    assert _args.occupancy_start(np.array([-7, 3], np.int16), B, S, np.float32)[0].tolist() == [-1, 3]
    idx, mu0 = _args.occupancy_start(np.ones((B, 2 * S))[:, ::2], B, S, np.float32)
    assert idx is None and mu0.dtype == np.float32 and mu0.flags.c_contiguous and mu0.shape == (B, S)
    for bad in (np.zeros(3, np.int32), np.zeros(B, np.float64), np.zeros((B, 99))):
        with pytest.raises(ValueError, match=r"start of shape \(\d+(, \d+)?,?\) is neither \(2,\) state indices nor a \(2, 100\) array"):
            _args.occupancy_start(bad, B, S, np.float64)


# ---------------------------------------------------------------- the other MiniGridVecEnv rules
def test_rollout_budget():
    assert _args.rollout_budget(None) == 0 and _args.rollout_budget(np.int64(12)) == 12
    for bad in (0, -1):
        with pytest.raises(ValueError, match=r"max_steps must be > 0 \(None: no budget\)"):
            _args.rollout_budget(bad)


def test_trace_arrays():
    assert _args.trace_arrays(False, 50, 0, B) == (None, None, 0) and _args.trace_arrays(0, 50, 0, B) == (None, None, 0)
    for trace, cap, n in ((True, 0, 50), (True, 20, 20), (7, 20, 7), (30, 20, 20), (30, 0, 30)):
        ts, ta, tlen = _args.trace_arrays(trace, 50, cap, B)
        assert tlen == n and ts.shape == ta.shape == (n, B) and ts.dtype == np.int32 and ta.dtype == np.int8
    with pytest.raises(ValueError, match="trace must be True, False or a positive number of steps"):
        _args.trace_arrays(-2, 50, 0, B)


def test_seed_args():
    assert _args.seed_args(np.int64(7), None, B) == (7, None)
    seed, mask = _args.seed_args(2 ** 64 - B, [[True], [False]], B)
    assert seed == 2 ** 64 - B and mask.dtype == np.uint8 and mask.shape == (B,) and mask.tolist() == [1, 0]
    for bad in (2 ** 64 - B + 1, -1):
        with pytest.raises(ValueError, match=r"seed \.\. seed \+ 2 must fit 64 bits \(one SeedSequence entropy int each\)"):
            _args.seed_args(bad, None, B)


def test_slip_random_action():
    assert _args.slip_random_action(None) == -1 and _args.slip_random_action(0) == 0 and _args.slip_random_action(6) == 6
    with pytest.raises(ValueError, match="random_action must be an env action 0..6 or None, got -1"):
        _args.slip_random_action(-1)


def test_q_n_act():
    assert _args.q_n_act(None, A, "xyd") == A and _args.q_n_act(3, A, "xyd") == 3 and _args.q_n_act(5, 5, "doorkey") == 5
    for bad, lanes, model in ((0, 7, "xyd"), (8, 7, "xyd"), (6, 5, "doorkey")):
        with pytest.raises(ValueError, match=rf"n_act must be in 1\.\.{lanes} for the {model} model, got {bad}"):
            _args.q_n_act(bad, lanes, model)


def test_q_table():
    z = _args.q_table(None, B, S, A)
    assert z.dtype == np.float64 and z.shape == (B, S, A) and not z.any()
    Q = np.arange(B * S * A, dtype=np.float64).reshape(B, S, A)
    q = _args.q_table(Q, B, S, A)
    assert q is not Q and not np.shares_memory(q, Q) and q.flags.c_contiguous and np.array_equal(q, Q)
    q[0, 0, 0] = -1.0  # the caller's table stays as it is
    assert Q[0, 0, 0] == 0.0
    assert _args.q_table(np.asfortranarray(Q), B, S, A).flags.c_contiguous
    with pytest.raises(ValueError, match=r"Q must be float64 \(fp32 tables are out of scope\), got dtype float32"):
        _args.q_table(Q.astype(np.float32), B, S, A)
    with pytest.raises(ValueError, match=r"Q of shape \(2, 100, 5\) is not \(2, 100, 7\)"):
        _args.q_table(Q[:, :, :5], B, S, A)


def test_q_params():
    assert _args.q_params(np.int64(10), 1, 0.5, 0) == (10, 1.0, 0.5, 0.0)
    assert _args.q_params(2 ** 31 - 1, 0.5, 0.99, 1.0)[0] == 2 ** 31 - 1
    for bad in (0, -4):
        with pytest.raises(ValueError, match=f"n_steps must be > 0, got {bad}"):
            _args.q_params(bad, 0.5, 0.99, 0.1)
    with pytest.raises(ValueError, match="n_steps must fit int32"):
        _args.q_params(2 ** 31, 0.5, 0.99, 0.1)
    for bad in (float("nan"), 1.5, -0.1):
        with pytest.raises(ValueError, match=r"eps must be in \[0, 1\], got"):
            _args.q_params(10, 0.5, 0.99, bad)
    for alpha, gamma in ((float("nan"), 0.99), (0.5, float("nan"))):
        with pytest.raises(ValueError, match="alpha and gamma must not be NaN"):
            _args.q_params(10, alpha, gamma, 0.1)
