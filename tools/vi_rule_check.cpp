// vi_rule_check -- drive the global stopping rule (csrc/vi_rule.h) with scripted dV traces (host only, no GPU).
//
//   g++ -std=c++17 -I minigrid_dynamicprogramming_amd/csrc tools/vi_rule_check.cpp -o vi_rule_check
//
// Each input line: tol max_sweeps horizon K fail_at fail_code reduce null_out dV(1) dV(2) ...
//   K         the common sweep the closing steps start from, with dV(K) from the trace (the last entry
//             repeats past its end; "nan" is a NaN)
//   fail_at   the sweep whose step returns fail_code instead of sweeping (0 = none)
//   reduce    1 = the step also calls a "reduce" hook behind its sweep (the sharded solve's all-reduce)
//   null_out  1 = the report gets null out-parameters
// Each output line: rc k dv converged sweeps_out dv_out converged_out : the calls in order (s<k> a sweep
// to k, r<k> the hook behind it).  On rc != 0 nothing is reported (converged and the outs print as -1).
// tests/test_vi_rule_cpu.py builds this with -fsanitize=address,undefined and checks the lines.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "vi_rule.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        std::vector<double> f;
        for (std::string tok; in >> tok;) f.push_back(std::strtod(tok.c_str(), nullptr));
        if (f.size() < 9) {
            std::fprintf(stderr, "bad row: %s\n", line.c_str());
            return 2;
        }
        const double tol = f[0];
        const int32_t max_sweeps = (int32_t)f[1];
        const int horizon = (int)f[2], fail_at = (int)f[4], fail_code = (int)f[5];
        const bool reduce = f[6] != 0, null_out = f[7] != 0;
        const std::vector<double> trace(f.begin() + 8, f.end());
        auto dv_at = [&](int32_t k) { return trace[(size_t)k <= trace.size() ? (size_t)k - 1 : trace.size() - 1]; };
        int32_t k = (int32_t)f[3];
        if (k < 1) {
            std::fprintf(stderr, "bad row (K < 1): %s\n", line.c_str());
            return 2;
        }
        double dv = dv_at(k);
        std::string log;
        const int rc = mgdp::rule_sweeps(tol, max_sweeps, &k, &dv, [&](int32_t k1, double *d) {
            log += " s" + std::to_string(k1);
            if (k1 == fail_at) return fail_code;
            *d = dv_at(k1);
            if (reduce) log += " r" + std::to_string(k1);
            return 0;
        });
        int32_t converged = -1, sweeps_out = -1, converged_out = -1;
        double dv_out = -1.0;
        if (rc == 0)
            converged = null_out ? mgdp::rule_report(horizon, tol, k, dv, nullptr, nullptr, nullptr)
                                 : mgdp::rule_report(horizon, tol, k, dv, &sweeps_out, &dv_out, &converged_out);
        std::printf("%d %d %.17g %d %d %.17g %d :%s\n", rc, k, dv, converged, sweeps_out, dv_out, converged_out, log.c_str());
    }
    return 0;
}
