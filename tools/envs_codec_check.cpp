// envs_codec_check -- drive the env half's cell codec (csrc/envs_codec.h) from stdin (host only, no GPU).
//
//   g++ -std=c++17 -I minigrid_dynamicprogramming_amd/csrc tools/envs_codec_check.cpp -o envs_codec_check
//
// One command per run: a word, then whitespace-separated integers.  Every array is exactly as long as
// the header is told it is (heap blocks of that size, so a walk that leaves one is a sanitizer report).
//   encode B W H HWp M mask[B if M] enc[B*W*H*3]            -> "ok" plane[B*HWp]        | "err kind carried b x y t c s"
//   decode B W H HWp plane[B*HWp]                           -> enc[B*W*H*3]
//   contents B W H HWp cells[B*HWp] contents[B*W*H*3]       -> "ok" plane[B*HWp]        | "err ..."
//   uncontents B W H HWp plane[B*HWp]                       -> contents[B*W*H*3]
//   carried B carry[B*2] triples[B*3]                       -> "ok" codes[B]            | "err ..."
//   uncarried B codes[B]                                    -> triples[B*3]
//   agent W H x y d                                         -> 0 | 1
//   stage B HWp                                             -> mask see cells agent carry max total
// kind: 1 not a Grid.encode() cell, 2 not an object a Box can hold, 3 an object not on a Box.
// tests/test_envs_codec_cpu.py builds this with -fsanitize=address,undefined and checks the lines.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "envs_codec.h"

namespace {

template <typename T>
std::vector<T> take(size_t n) {
    std::vector<T> v(n);
    for (auto &x : v) {
        long long t;
        if (!(std::cin >> t)) {
            std::fprintf(stderr, "short input\n");
            std::exit(2);
        }
        x = (T)t;
    }
    return v;
}
int take1() { return take<int>(1)[0]; }

template <typename T>
void put(const char *head, const std::vector<T> &v) {
    std::printf("%s", head);
    for (auto x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

int report(const mgdp::CodecError &e, const std::vector<uint8_t> &out) {
    if (e) std::printf("err %d %d %d %d %d %d %d %d\n", (int)e.kind, (int)e.carried, e.b, e.x, e.y, e.t, e.c, e.s);
    else put("ok", out);
    return 0;
}

mgdp::BatchShape take_shape() {
    const int B = take1(), W = take1(), H = take1(), HWp = take1();
    return mgdp::BatchShape{B, W, H, HWp};
}

}  // namespace

int main() {
    std::string cmd;
    std::cin >> cmd;
    if (cmd == "encode") {
        const mgdp::BatchShape g = take_shape();
        const auto mask = take<uint8_t>(take1() ? g.B : 0);
        const auto enc = take<uint8_t>((size_t)g.B * g.W * g.H * 3);
        std::vector<uint8_t> plane((size_t)g.B * g.HWp, 0xEE);
        return report(mgdp::encode_cells(g, enc.data(), mask.empty() ? nullptr : mask.data(), plane.data()), plane);
    }
    if (cmd == "decode" || cmd == "uncontents") {
        const mgdp::BatchShape g = take_shape();
        const auto plane = take<uint8_t>((size_t)g.B * g.HWp);
        std::vector<uint8_t> enc((size_t)g.B * g.W * g.H * 3, 0xEE);
        if (cmd == "decode") mgdp::decode_cells(g, plane.data(), enc.data());
        else mgdp::decode_contents(g, plane.data(), enc.data());
        put("", enc);
        return 0;
    }
    if (cmd == "contents") {
        const mgdp::BatchShape g = take_shape();
        const auto cells = take<uint8_t>((size_t)g.B * g.HWp);
        const auto contents = take<uint8_t>((size_t)g.B * g.W * g.H * 3);
        std::vector<uint8_t> plane((size_t)g.B * g.HWp, 0xEE);
        return report(mgdp::encode_contents(g, contents.data(), cells.data(), plane.data()), plane);
    }
    if (cmd == "carried") {
        const int B = take1();
        const auto carry = take<int32_t>((size_t)B * 2), triples = take<int32_t>((size_t)B * 3);
        std::vector<uint8_t> codes((size_t)B, 0xEE);
        return report(mgdp::encode_carried(B, triples.data(), carry.data(), codes.data()), codes);
    }
    if (cmd == "uncarried") {
        const int B = take1();
        const auto codes = take<uint8_t>((size_t)B);
        std::vector<int32_t> triples((size_t)B * 3, -1);
        mgdp::decode_carried(B, codes.data(), triples.data());
        put("", triples);
        return 0;
    }
    if (cmd == "agent") {
        const int W = take1(), H = take1(), x = take1(), y = take1(), d = take1();
        std::printf("%d\n", (int)mgdp::agent_in_grid(x, y, d, W, H));
        return 0;
    }
    if (cmd == "stage") {
        const int B = take1(), HWp = take1();
        const mgdp::StageLayout L{B, HWp};
        std::vector<uint8_t> buf(L.total());  // each section's first byte is inside it
        const uint8_t *st = buf.data();
        auto off = [&](const void *p) { return (size_t)(static_cast<const uint8_t *>(p) - st); };
        put("", std::vector<size_t>{off(&st[L.mask(0)]), off(&st[L.see(0)]), off(L.cells(st)), off(L.agent(st)), off(L.carry(st)),
                                    off(L.max(st)), L.total()});
        return 0;
    }
    std::fprintf(stderr, "unknown command: %s\n", cmd.c_str());
    return 2;
}
