"""The value-iteration plan (csrc/vi_plan.h): which loop a handle runs, its workgroup and its LDS bytes.

The plan is host-plain C++, so it is checked without a GPU: tools/vi_plan_dump.cpp (its own main,
nothing but vi_plan.h) is built with the host compiler under AddressSanitizer + UBSan, run on every
row of TABLE and compared with it.  On the GPU the same rows are created as handles and must report
the same names.

TABLE was captured from handles of the commit before the plan existed (279c4c4), one process on an
MI355X: variant / kernel / persistent from vi.variant, vi.kernel_name, vi.persistent; block and
fused LDS bytes from the MGDP_DEBUG_OCC line of one launch-path solve with MGDP_PERSISTENT=0 added
(None where that build printed none: the options and sweep kernels).
"""
import ctypes
import os
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "minigrid_dynamicprogramming_amd", "csrc")

# model, dtype, method, mapping, B, W, H, slip_p, horizon, lava_mode, flags, knobs,
#   variant, kernel, persistent, block, fused LDS bytes
TABLE = [
    (0, 0, 0, 0, 1, 5, 5, -1.0, 0, 0, 0, "", "serve_wave", "vi_serve_kernel", True, 64, 2656),
    (0, 0, 0, 0, 1, 8, 8, -1.0, 0, 0, 0, "", "serve_wave", "vi_serve_kernel", True, 64, 2688),
    (0, 0, 0, 0, 1, 9, 9, -1.0, 0, 0, 0, "", "serve_pair", "vi_serve_kernel", True, 128, 7072),
    (0, 0, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "", "serve_pair", "vi_serve_kernel", True, 256, 13888),
    (0, 0, 0, 0, 1, 19, 19, -1.0, 0, 0, 0, "", "serve", "vi_serve_kernel", True, 384, 14512),
    (0, 0, 0, 0, 1, 33, 33, -1.0, 0, 0, 0, "", "xyd_soa", "vi_fused_kernel", False, 1024, 40640),
    (0, 0, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_SERVE_PAIR=0", "serve_ew", "vi_serve_kernel", True, 256, 9792),
    (0, 0, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_SERVE_EW=0", "serve", "vi_serve_kernel", True, 256, 9792),
    (0, 0, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE=8", "serve_wave", "vi_serve_kernel", True, 64, 9792),
    (0, 0, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_LONE_CPT=2", "serve", "vi_serve_kernel", True, 128, 9792),
    (0, 0, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_SERVE_BAND=1", "serve_band", "vi_serve_kernel", True, 64, 512),
    (0, 0, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_PERSISTENT=0", "xyd_soa", "vi_fused_kernel", False, 256, 13888),
    (0, 0, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_PAIR=1", "pair", "vi_fused_kernel", False, 256, 13888),
    (0, 0, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_QUAD=1", "quad", "vi_fused_kernel", False, 1024, 9792),
    (0, 0, 0, 0, 1, 8, 8, -1.0, 0, 0, 0, "MGDP_PAIR=1", "pair", "vi_fused_kernel", False, 64, 3712),
    (0, 0, 0, 0, 1, 8, 8, -1.0, 0, 0, 0, "MGDP_QUAD=1", "quad", "vi_fused_kernel", False, 256, 2688),
    (0, 0, 0, 0, 1, 23, 23, -1.0, 0, 0, 0, "MGDP_WAVE=8", "serve", "vi_serve_kernel", True, 576, 21600),
    (0, 0, 0, 0, 1, 23, 23, -1.0, 0, 0, 0, "MGDP_LONE_CPT=2", "serve", "vi_serve_kernel", True, 320, 23904),
    (0, 0, 0, 0, 1, 5, 5, 0.1, 0, 0, 0, "", "serve_wave", "vi_serve_kernel", True, 64, 2656),
    (0, 0, 0, 0, 1, 16, 16, 0.1, 0, 0, 0, "", "serve", "vi_serve_kernel", True, 256, 9792),
    (0, 0, 0, 0, 1, 16, 16, 0.1, 0, 0, 0, "MGDP_LONE_CPT=2", "serve", "vi_serve_kernel", True, 128, 9792),
    (0, 0, 0, 0, 8, 5, 5, -1.0, 0, 0, 0, "", "wave2", "vi_fused_kernel", False, 64, 928),
    (0, 0, 0, 0, 8, 11, 11, -1.0, 0, 0, 0, "", "wave2", "vi_fused_kernel", False, 64, 1536),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "", "wave2", "vi_fused_kernel", False, 64, 2688),
    (0, 0, 0, 0, 8, 19, 19, -1.0, 0, 0, 0, "", "wave2", "vi_fused_kernel", False, 64, 3952),
    (0, 0, 0, 0, 8, 23, 23, -1.0, 0, 0, 0, "", "xyd_pair2", "vi_fused_kernel", False, 320, 23904),
    (0, 0, 0, 0, 8, 33, 33, -1.0, 0, 0, 0, "", "xyd_soa", "vi_fused_kernel", False, 1024, 40640),
    (0, 0, 0, 0, 8, 16, 16, 0.1, 0, 0, 0, "", "xyd_x2", "vi_fused_kernel", False, 128, 9792),
    (0, 0, 0, 0, 8, 23, 23, 0.1, 0, 0, 0, "", "xyd_x2", "vi_fused_kernel", False, 320, 23904),
    (0, 0, 0, 0, 8, 23, 23, -1.0, 0, 0, 0, "MGDP_PAIR2=0", "xyd_x2", "vi_fused_kernel", False, 320, 23904),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2=0", "xyd_pair2", "vi_fused_kernel", False, 128, 9792),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2=0 MGDP_CPT=1", "xyd_soa", "vi_fused_kernel", False, 256, 9792),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2=0 MGDP_CPT=4", "xyd_x4", "vi_fused_kernel", False, 64, 9792),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2=0 MGDP_PAIR2=0", "xyd_x2", "vi_fused_kernel", False, 128, 9792),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_PAIR=1", "pair", "vi_fused_kernel", False, 256, 13888),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_QUAD=1", "quad", "vi_fused_kernel", False, 1024, 9792),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2N=1", "wave2n", "vi_fused_kernel", False, 128, 4928),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_MIX=1", "mix", "vi_fused_kernel", False, 128, 4928),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_BAND=1", "band", "vi_fused_kernel", False, 64, 512),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_GK=0", "wave2", "vi_fused_kernel", False, 64, 2688),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_GK=1", "wave2", "vi_fused_kernel", False, 64, 2688),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_BSERVE=0", "wave2", "vi_fused_kernel", False, 64, 2688),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_BSERVE=2", "wave2", "vi_fused_kernel", False, 64, 2688),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2=2", "xyd_pair2", "vi_fused_kernel", False, 128, 9792),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2N=1 MGDP_MIX=1", "wave2n", "vi_fused_kernel", False, 128, 4928),
    (0, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2N=1 MGDP_BAND=1", "wave2n", "vi_fused_kernel", False, 128, 4928),
    (0, 0, 0, 0, 8, 8, 8, -1.0, 0, 0, 0, "MGDP_QUAD=1", "quad", "vi_fused_kernel", False, 256, 2688),
    (0, 0, 0, 0, 8, 11, 11, -1.0, 0, 0, 0, "MGDP_WAVE2N=1", "wave2", "vi_fused_kernel", False, 64, 1536),
    (0, 0, 0, 0, 8, 11, 11, -1.0, 0, 0, 0, "MGDP_MIX=1", "mix", "vi_fused_kernel", False, 128, 2752),
    (0, 0, 0, 0, 8, 5, 5, -1.0, 0, 0, 0, "MGDP_MIX=1", "wave2", "vi_fused_kernel", False, 64, 928),
    (1, 0, 0, 0, 1, 8, 8, -1.0, 0, 0, 0, "", "serve_dk_half", "vi_serve_kernel", True, 128, 9600),
    (1, 0, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "", "serve_dk_half", "vi_serve_kernel", True, 512, 37440),
    (1, 0, 0, 0, 8, 8, 8, -1.0, 0, 0, 0, "", "dk_soa", "vi_fused_kernel", False, 64, 9600),
    (1, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "", "dk_rows", "vi_fused_kernel", False, 256, 19136),
    (1, 0, 0, 0, 8, 16, 24, -1.0, 0, 0, 0, "", "dk_rows", "vi_fused_kernel", False, 384, 27456),
    (1, 0, 0, 0, 8, 24, 24, -1.0, 0, 0, 0, "", "dk_soa", "vi_fused_kernel", False, 576, 83840),
    (1, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_DK_ROWS=0", "dk_soa", "vi_fused_kernel", False, 256, 37440),
    (1, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_DK_HALF=1", "dk_half", "vi_fused_kernel", False, 512, 37440),
    (1, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_DK_HALF=0", "dk_rows", "vi_fused_kernel", False, 256, 19136),
    (1, 0, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_DK_1T=1", "dk_1t", "vi_fused_kernel", False, 256, 21056),
    (1, 0, 0, 0, 1, 8, 8, -1.0, 0, 0, 0, "MGDP_DK_HALF=0", "serve", "vi_serve_kernel", True, 64, 9600),
    (0, 0, 0, 0, 8, 9, 9, -1.0, 16, 0, 0, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (0, 0, 0, 0, 8, 9, 9, -1.0, 16, 0, 1, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (0, 0, 0, 0, 8, 9, 9, -1.0, 0, 1, 0, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (0, 0, 0, 0, 8, 9, 9, 0.1, 0, 1, 0, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (0, 0, 0, 0, 1, 9, 9, -1.0, 0, 1, 0, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (1, 0, 0, 0, 8, 8, 8, -1.0, 16, 0, 0, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (0, 0, 0, 1, 1, 8, 8, -1.0, 0, 0, 0, "", "sa", "vi_fused_kernel", False, 1024, 2688),
    (0, 0, 0, 1, 8, 8, 8, -1.0, 0, 0, 0, "", "sa", "vi_fused_kernel", False, 256, 2688),
    (0, 0, 1, 0, 8, 16, 16, -1.0, 0, 0, 0, "", "sweep_pipe", "vi_sweep_pipe_kernel", False, None, None),
    (1, 0, 1, 0, 8, 8, 8, -1.0, 0, 0, 0, "", "sweep", "vi_sweep_kernel", False, None, None),
    (0, 0, 1, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_SWEEP_PIPE=0", "sweep", "vi_sweep_kernel", False, None, None),
    (0, 0, 1, 0, 8, 33, 33, -1.0, 0, 0, 0, "", "sweep", "vi_sweep_kernel", False, None, None),
    (0, 0, 1, 1, 8, 8, 8, -1.0, 0, 0, 0, "", "sweep", "vi_sweep_kernel", False, None, None),
    (0, 1, 0, 0, 1, 5, 5, -1.0, 0, 0, 0, "", "serve_wave", "vi_serve_kernel", True, 64, 4704),
    (0, 1, 0, 0, 1, 8, 8, -1.0, 0, 0, 0, "", "serve_wave", "vi_serve_kernel", True, 64, 4736),
    (0, 1, 0, 0, 1, 9, 9, -1.0, 0, 0, 0, "", "serve_pair", "vi_serve_kernel", True, 128, 13216),
    (0, 1, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "", "serve_pair", "vi_serve_kernel", True, 256, 26176),
    (0, 1, 0, 0, 1, 19, 19, -1.0, 0, 0, 0, "", "serve", "vi_serve_kernel", True, 384, 26800),
    (0, 1, 0, 0, 1, 33, 33, -1.0, 0, 0, 0, "", "xyd_soa", "vi_fused_kernel", False, 1024, 75488),
    (0, 1, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_SERVE_PAIR=0", "serve_ew", "vi_serve_kernel", True, 256, 17984),
    (0, 1, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_SERVE_EW=0", "serve", "vi_serve_kernel", True, 256, 17984),
    (0, 1, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE=8", "serve_wave", "vi_serve_kernel", True, 64, 17984),
    (0, 1, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_LONE_CPT=2", "serve", "vi_serve_kernel", True, 128, 17984),
    (0, 1, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_SERVE_BAND=1", "serve_band", "vi_serve_kernel", True, 64, 512),
    (0, 1, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_PERSISTENT=0", "xyd_soa", "vi_fused_kernel", False, 256, 26176),
    (0, 1, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_PAIR=1", "pair", "vi_fused_kernel", False, 256, 26176),
    (0, 1, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "MGDP_QUAD=1", "quad", "vi_fused_kernel", False, 1024, 17984),
    (0, 1, 0, 0, 1, 8, 8, -1.0, 0, 0, 0, "MGDP_PAIR=1", "pair", "vi_fused_kernel", False, 64, 6784),
    (0, 1, 0, 0, 1, 8, 8, -1.0, 0, 0, 0, "MGDP_QUAD=1", "quad", "vi_fused_kernel", False, 256, 4736),
    (0, 1, 0, 0, 1, 23, 23, -1.0, 0, 0, 0, "MGDP_WAVE=8", "serve", "vi_serve_kernel", True, 576, 40032),
    (0, 1, 0, 0, 1, 23, 23, -1.0, 0, 0, 0, "MGDP_LONE_CPT=2", "serve", "vi_serve_kernel", True, 320, 44384),
    (0, 1, 0, 0, 1, 5, 5, 0.1, 0, 0, 0, "", "serve_wave", "vi_serve_kernel", True, 64, 4704),
    (0, 1, 0, 0, 1, 16, 16, 0.1, 0, 0, 0, "", "serve", "vi_serve_kernel", True, 256, 17984),
    (0, 1, 0, 0, 1, 16, 16, 0.1, 0, 0, 0, "MGDP_LONE_CPT=2", "serve", "vi_serve_kernel", True, 128, 17984),
    (0, 1, 0, 0, 8, 5, 5, -1.0, 0, 0, 0, "", "wave2", "vi_fused_kernel", False, 64, 1568),
    (0, 1, 0, 0, 8, 11, 11, -1.0, 0, 0, 0, "", "wave2", "vi_fused_kernel", False, 64, 2688),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "", "wave2", "vi_fused_kernel", False, 64, 4864),
    (0, 1, 0, 0, 8, 19, 19, -1.0, 0, 0, 0, "", "wave2", "vi_fused_kernel", False, 64, 7280),
    (0, 1, 0, 0, 8, 23, 23, -1.0, 0, 0, 0, "", "xyd_pair2", "vi_fused_kernel", False, 320, 44384),
    (0, 1, 0, 0, 8, 33, 33, -1.0, 0, 0, 0, "", "xyd_soa", "vi_fused_kernel", False, 1024, 75488),
    (0, 1, 0, 0, 8, 16, 16, 0.1, 0, 0, 0, "", "xyd_x2", "vi_fused_kernel", False, 128, 17984),
    (0, 1, 0, 0, 8, 23, 23, 0.1, 0, 0, 0, "", "xyd_x2", "vi_fused_kernel", False, 320, 44384),
    (0, 1, 0, 0, 8, 23, 23, -1.0, 0, 0, 0, "MGDP_PAIR2=0", "xyd_x2", "vi_fused_kernel", False, 320, 44384),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2=0", "xyd_pair2", "vi_fused_kernel", False, 128, 17984),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2=0 MGDP_CPT=1", "xyd_soa", "vi_fused_kernel", False, 256, 17984),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2=0 MGDP_CPT=4", "xyd_x4", "vi_fused_kernel", False, 64, 17984),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2=0 MGDP_PAIR2=0", "xyd_x2", "vi_fused_kernel", False, 128, 17984),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_PAIR=1", "pair", "vi_fused_kernel", False, 256, 26176),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_QUAD=1", "quad", "vi_fused_kernel", False, 1024, 17984),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2N=1", "wave2n", "vi_fused_kernel", False, 128, 9280),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_MIX=1", "wave2", "vi_fused_kernel", False, 64, 4864),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_BAND=1", "band", "vi_fused_kernel", False, 64, 512),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_GK=0", "wave2", "vi_fused_kernel", False, 64, 4864),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_GK=1", "wave2", "vi_fused_kernel", False, 64, 4864),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_BSERVE=0", "wave2", "vi_fused_kernel", False, 64, 4864),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_BSERVE=2", "wave2", "vi_fused_kernel", False, 64, 4864),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2=2", "xyd_pair2", "vi_fused_kernel", False, 128, 17984),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2N=1 MGDP_MIX=1", "wave2n", "vi_fused_kernel", False, 128, 9280),
    (0, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_WAVE2N=1 MGDP_BAND=1", "wave2n", "vi_fused_kernel", False, 128, 9280),
    (0, 1, 0, 0, 8, 8, 8, -1.0, 0, 0, 0, "MGDP_QUAD=1", "quad", "vi_fused_kernel", False, 256, 4736),
    (0, 1, 0, 0, 8, 11, 11, -1.0, 0, 0, 0, "MGDP_WAVE2N=1", "wave2", "vi_fused_kernel", False, 64, 2688),
    (0, 1, 0, 0, 8, 11, 11, -1.0, 0, 0, 0, "MGDP_MIX=1", "wave2", "vi_fused_kernel", False, 64, 2688),
    (0, 1, 0, 0, 8, 5, 5, -1.0, 0, 0, 0, "MGDP_MIX=1", "wave2", "vi_fused_kernel", False, 64, 1568),
    (1, 1, 0, 0, 1, 8, 8, -1.0, 0, 0, 0, "", "serve_dk_half", "vi_serve_kernel", True, 128, 17792),
    (1, 1, 0, 0, 1, 16, 16, -1.0, 0, 0, 0, "", "serve_dk_half", "vi_serve_kernel", True, 512, 70208),
    (1, 1, 0, 0, 8, 8, 8, -1.0, 0, 0, 0, "", "dk_half", "vi_fused_kernel", False, 128, 17792),
    (1, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "", "dk_half", "vi_fused_kernel", False, 512, 70208),
    (1, 1, 0, 0, 8, 16, 24, -1.0, 0, 0, 0, "", "dk_half", "vi_fused_kernel", False, 768, 105152),
    (1, 1, 0, 0, 8, 24, 24, -1.0, 0, 0, 0, "", "dk_soa", "vi_fused_kernel", False, 576, 157568),
    (1, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_DK_ROWS=0", "dk_half", "vi_fused_kernel", False, 512, 70208),
    (1, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_DK_HALF=1", "dk_half", "vi_fused_kernel", False, 512, 70208),
    (1, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_DK_HALF=0", "dk_rows", "vi_fused_kernel", False, 256, 37568),
    (1, 1, 0, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_DK_1T=1", "dk_half", "vi_fused_kernel", False, 512, 70208),
    (1, 1, 0, 0, 1, 8, 8, -1.0, 0, 0, 0, "MGDP_DK_HALF=0", "serve", "vi_serve_kernel", True, 64, 17792),
    (0, 1, 0, 0, 8, 9, 9, -1.0, 16, 0, 0, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (0, 1, 0, 0, 8, 9, 9, -1.0, 16, 0, 1, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (0, 1, 0, 0, 8, 9, 9, -1.0, 0, 1, 0, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (0, 1, 0, 0, 8, 9, 9, 0.1, 0, 1, 0, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (0, 1, 0, 0, 1, 9, 9, -1.0, 0, 1, 0, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (1, 1, 0, 0, 8, 8, 8, -1.0, 16, 0, 0, "", "opts", "vi_fused_opts_kernel", False, None, None),
    (0, 1, 0, 1, 1, 8, 8, -1.0, 0, 0, 0, "", "sa", "vi_fused_kernel", False, 1024, 4736),
    (0, 1, 0, 1, 8, 8, 8, -1.0, 0, 0, 0, "", "sa", "vi_fused_kernel", False, 256, 4736),
    (0, 1, 1, 0, 8, 16, 16, -1.0, 0, 0, 0, "", "sweep_pipe", "vi_sweep_pipe_kernel", False, None, None),
    (1, 1, 1, 0, 8, 8, 8, -1.0, 0, 0, 0, "", "sweep", "vi_sweep_kernel", False, None, None),
    (0, 1, 1, 0, 8, 16, 16, -1.0, 0, 0, 0, "MGDP_SWEEP_PIPE=0", "sweep", "vi_sweep_kernel", False, None, None),
    (0, 1, 1, 0, 8, 33, 33, -1.0, 0, 0, 0, "", "sweep", "vi_sweep_kernel", False, None, None),
    (0, 1, 1, 1, 8, 8, 8, -1.0, 0, 0, 0, "", "sweep", "vi_sweep_kernel", False, None, None),
]

KNOB_NAMES = sorted({kv.split("=")[0] for r in TABLE for kv in r[11].split()})


def _dump_lines():
    return ["%d %d %d %d %d %d %d %r %d %d %d %s" % r[:12] for r in TABLE]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vi_plan") / "vi_plan_dump")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tools", "vi_plan_dump.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def plan_dump(plan_exe):
    r = subprocess.run([plan_exe], input="\n".join(_dump_lines()) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = [line.split() for line in r.stdout.splitlines()]
    assert len(out) == len(TABLE)
    return out


def test_plan_names_match_the_captured_table(plan_dump):
    for row, (variant, kernel, served, *_rest) in zip(TABLE, plan_dump):
        assert (variant, kernel, bool(int(served))) == row[12:15], row


def test_plan_launch_shape_matches_the_captured_table(plan_dump):
    checked = 0
    for row, (_v, _k, served, block, _hws, _nbuf, lds, serve_lds) in zip(TABLE, plan_dump):
        if row[15] is None:
            continue
        checked += 1
        assert (int(block), int(lds)) == row[15:17], row
        # every lone-grid server but the column-band one keeps the fused launch's usual layout
        if int(served) and row[12] != "serve_band":
            assert int(serve_lds) == row[16], row
    assert checked >= 120


def test_plan_ignores_mix_for_fp64(plan_dump):
    got = {(r[1], r[11]): p[0] for r, p in zip(TABLE, plan_dump) if r[4:7] == (8, 16, 16) and r[0] == 0 and r[2] == 0}
    assert got[(0, "MGDP_MIX=1")] == "mix" and got[(1, "MGDP_MIX=1")] == "wave2"


def test_dump_refuses_an_unknown_knob(plan_exe):
    """The knob table is the only way in: a name it does not hold is an error, not a silent default."""
    r = subprocess.run([plan_exe], input="0 0 0 0 8 16 16 -1.0 0 0 0 MGDP_NO_SUCH_KNOB=1\n", capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "MGDP_NO_SUCH_KNOB" in r.stderr


@pytest.mark.gpu
def test_handles_report_the_planned_names(monkeypatch):
    from minigrid_dynamicprogramming_amd import _lib

    L = _lib.load()
    _lib.require_gpu()
    bad = []
    for row in TABLE:
        for name in KNOB_NAMES:
            monkeypatch.delenv(name, raising=False)
        for kv in row[11].split():
            monkeypatch.setenv(*kv.split("="))
        d = _lib.ViDesc()
        d.model, d.dtype, d.method, d.mapping, d.B, d.W, d.H = row[:7]
        d.slip_p, d.horizon, d.lava_mode, d.flags = row[7:11]
        d.max_sweeps, d.gamma, d.tol, d.death_cost = 10000, 0.99, 1e-6, -1.0
        h = ctypes.c_void_p()
        _lib.check(L.mgdp_vi_create(ctypes.byref(d), ctypes.byref(h)), "mgdp_vi_create")
        try:
            on = ctypes.c_int32(0)
            _lib.check(L.mgdp_vi_persistent(h, ctypes.byref(on)), "mgdp_vi_persistent")
            got = (L.mgdp_vi_variant(h).decode(), L.mgdp_vi_kernel_name(h).decode(), bool(on.value))
        finally:
            L.mgdp_vi_destroy(h)
        if got != row[12:15]:
            bad.append((row[:12], got, row[12:15]))
    assert not bad, bad
