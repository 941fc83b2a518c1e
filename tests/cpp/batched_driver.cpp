// Test driver of ccp::SolveWeighted's channels parameter (include/ccp/photomontage.h): sees only the facade and the C ABI.
//   batched_driver <default|sequential|batched> <iterations> <in> <out>
// default: the call without the trailing parameter; every call uses Hierarchy::Rescaled and Precision::Double.  in / out:
// weighted_driver.cpp's files (int32 W, H, C, then int32 presence flags of gx, gy, f, wx, wy, lambda, then the present
// float32 arrays; out: the H x W x C u8 result).  Exit 2 on a throw, with the message on stderr.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ccp/photomontage.h"

int main(int argc, char **argv)
{
    if (argc != 5) return 1;
    const std::string channels = argv[1];
    if (channels != "default" && channels != "sequential" && channels != "batched") return 1;
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
    try {
        if (channels == "default")
            ccp::SolveWeighted(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ov, iterations, ccp::Solver::MultigridConjugateGradient, 0,
                               ccp::Hierarchy::Rescaled, ccp::Precision::Double);
        else
            ccp::SolveWeighted(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ov, iterations, ccp::Solver::MultigridConjugateGradient, 0,
                               ccp::Hierarchy::Rescaled, ccp::Precision::Double,
                               channels == "batched" ? ccp::Channels::Batched : ccp::Channels::Sequential);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
    return 0;
}
