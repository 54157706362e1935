// vi_plan_dump -- print the value-iteration plan of descriptors read from stdin (host only, no GPU).
//
//   g++ -std=c++17 -I minigrid_dynamicprogramming_amd/csrc tools/vi_plan_dump.cpp -o vi_plan_dump
//
// Each input line: model dtype method mapping B W H slip_p horizon lava_mode flags [MGDP_NAME=value ...]
// (the integer codes of include/mgdp.h).  Each output line:
//   variant kernel persistent block HWs nbuf fused_lds serve_lds
// tests/test_vi_plan.py builds this with -fsanitize=address,undefined and compares it with a table
// captured from handles on the GPU.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "vi_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        mgdp_vi_desc d{};
        in >> d.model >> d.dtype >> d.method >> d.mapping >> d.B >> d.W >> d.H >> d.slip_p >> d.horizon >> d.lava_mode >> d.flags;
        if (!in) {
            std::fprintf(stderr, "bad row: %s\n", line.c_str());
            return 2;
        }
        mgdp::ViKnobs kn;
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || !mgdp::set_knob(kn, kv.substr(0, eq).c_str(), kv.c_str() + eq + 1)) {
                std::fprintf(stderr, "unknown knob: %s\n", kv.c_str());
                return 2;
            }
        }
        const mgdp::ViPlan p = mgdp::plan_vi(d, kn);
        const bool served = kn.persistent && p.serve_shape;
        std::printf("%s %s %d %d %d %d %d %d\n", mgdp::variant_name(p, served), mgdp::kernel_name(p, served), (int)served,
                    p.block, p.HWs, p.nbuf, p.lds, p.serve_lds);
    }
    return 0;
}
