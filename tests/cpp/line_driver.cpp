// Test driver of the smoother parameter of ccp::SolveWeighted and ccp::SolveConstrained (include/ccp/photomontage.h):
// sees only the facade and the C ABI.
//   line_driver <default|point|line|line_batched|c_default|c_point|c_line|c_line_batched> <iterations> <in> <out>
// default: the call without the trailing parameter; every call uses Hierarchy::Rescaled and Precision::Double, and
// line_batched asks for Channels::Batched with Smoother::Line, which the solve refuses.  c_*: the same through
// SolveConstrained, with the canvas's outermost two rows and columns fixed at f's values.  in / out: weighted_driver.cpp's
// files (int32 W, H, C, then int32 presence flags of gx, gy, f, wx, wy, lambda, then the present float32 arrays; out: the
// H x W x C u8 result).  Exit 2 on a throw, with the message on stderr.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ccp/photomontage.h"

int main(int argc, char **argv)
{
    if (argc != 5) return 1;
    std::string mode = argv[1];
    const bool constrained = mode.rfind("c_", 0) == 0;
    if (constrained) mode = mode.substr(2);
    if (mode != "default" && mode != "point" && mode != "line" && mode != "line_batched") return 1;
    const int iterations = std::stoi(argv[2]);
    std::ifstream in(argv[3], std::ios::binary);
    int32_t head[9];
    in.read(reinterpret_cast<char *>(head), sizeof(head));
    const int W = head[0], H = head[1], C = head[2];
    std::vector<float> arr[6];
    ccp::ImageView views[6];
    const ccp::ImageView *ptr[6] = {};
    for (int i = 0; i < 6; ++i) {
        if (!head[3 + i]) continue;
        const int ch = i < 3 ? C : 1;
        arr[i].resize((size_t)W * H * ch);
        in.read(reinterpret_cast<char *>(arr[i].data()), (std::streamsize)(arr[i].size() * sizeof(float)));
        views[i] = ccp::ImageView{arr[i].data(), H, W, ch, (size_t)W * ch * sizeof(float)};
        ptr[i] = &views[i];
    }
    std::vector<uint8_t> out((size_t)W * H * C);
    ccp::ImageView ov{out.data(), H, W, C, (size_t)W * C};
    std::vector<uint8_t> mask((size_t)W * H, 0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) mask[(size_t)y * W + x] = x < 2 || y < 2 || x >= W - 2 || y >= H - 2;
    const ccp::ImageView fixed{mask.data(), H, W, 1, (size_t)W};
    const ccp::Channels channels = mode == "line_batched" ? ccp::Channels::Batched : ccp::Channels::Sequential;
    const ccp::Smoother smoother = mode == "point" ? ccp::Smoother::Point : ccp::Smoother::Line;
    try {
        if (constrained && mode == "default")
            ccp::SolveConstrained(ptr[0], ptr[1], ptr[2], ptr[2], fixed, ptr[3], ptr[4], ptr[5], ov, iterations, 0, ccp::Hierarchy::Rescaled,
                                  ccp::Precision::Double, ccp::Channels::Sequential);
        else if (constrained)
            ccp::SolveConstrained(ptr[0], ptr[1], ptr[2], ptr[2], fixed, ptr[3], ptr[4], ptr[5], ov, iterations, 0, ccp::Hierarchy::Rescaled,
                                  ccp::Precision::Double, channels, smoother);
        else if (mode == "default")
            ccp::SolveWeighted(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ov, iterations, ccp::Solver::MultigridConjugateGradient, 0,
                               ccp::Hierarchy::Rescaled, ccp::Precision::Double, ccp::Channels::Sequential);
        else
            ccp::SolveWeighted(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ov, iterations, ccp::Solver::MultigridConjugateGradient, 0,
                               ccp::Hierarchy::Rescaled, ccp::Precision::Double, channels, smoother);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
    return 0;
}
