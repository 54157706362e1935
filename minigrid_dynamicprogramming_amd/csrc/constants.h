// constants.h -- the reference's object, colour and door-state indices.  Plain C++17 (nothing from HIP):
// common.h hands them to every translation unit, envs_codec.h to a host compiler.
#pragma once

namespace mgdp {

// OBJECT_TO_IDX, minigrid/core/constants.py:25-37
enum : int {
    T_UNSEEN = 0, T_EMPTY = 1, T_WALL = 2, T_FLOOR = 3, T_DOOR = 4, T_KEY = 5, T_BALL = 6,
    T_BOX = 7, T_GOAL = 8, T_LAVA = 9, T_AGENT = 10
};
enum : int { C_GREY = 5 };                               // COLOR_TO_IDX, constants.py:20
enum : int { D_OPEN = 0, D_CLOSED = 1, D_LOCKED = 2 };   // STATE_TO_IDX, constants.py:42-46

}  // namespace mgdp
