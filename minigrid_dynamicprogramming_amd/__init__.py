"""MI355X-native Minigrid step + tabular value-iteration engine.

Hot path (HIP, gfx950, libmgdp.so behind include/mgdp.h):
  * MiniGridEnv.step / gen_obs for batches of envs            (csrc/envs.hip)
  * Jacobi value iteration over (pos, dir[, has_key, door_open]) (csrc/vi.hip: the C ABI over the
    host pieces csrc/vi_host*.h and the global stopping rule csrc/vi_rule.h)
  * policy evaluation (V^pi of a given policy), greedy improvement and policy iteration on the
    same model and stopping rule                              (csrc/vi_eval.h)
  * the same under NoDeath lava and finite horizons: V_0 and every V_t of a stationary or
    time-indexed policy in exactly H sweeps                   (csrc/vi_eval_opts.h)
  * the forward pass of a policy on the same options: state distribution, absorbed mass,
    discounted visitation and reward in exactly N steps       (csrc/vi_occupancy.h)
  * the action values Q(s, a) of a handle's V and the set of maximising actions per state, in
    q_learn's table layout                                    (csrc/vi_qvalues.h)
  * tabular policies executed on resident envs: policy lookup and the fused rollout, many steps
    of every env in one launch                                (csrc/envs_rollout.h)
Host side (this package): the reference's env API, registry and grid generators, the DP front end
and the multi-GPU driver.  See DESIGN.md.
"""
from .core import (COLOR_NAMES, COLOR_TO_IDX, DIR_TO_VEC, IDX_TO_COLOR, IDX_TO_OBJECT, OBJECT_TO_IDX,
                   STATE_TO_IDX, Actions, Ball, Box, Door, Floor, Goal, Grid, Key, Lava, Wall, WorldObj)
from .minigrid_env import MiniGridEnv, MissionSpace
from .envs import CrossingEnv, DistShiftEnv, DoorKeyEnv, EmptyEnv, FourRoomsEnv, LavaGapEnv
from .registry import EnvSpec, make, register, registry
from .dp import (ActionValues, OccupancyResult, ValueIteration, VIResult, action_values, policy_evaluation,
                 policy_iteration, policy_occupancy, value_iteration)
from .vector import MiniGridVecEnv, QLearnResult, RolloutResult

__version__ = "0.1.0"
