// Test driver of ccp::SolveConstrained (include/ccp/photomontage.h): sees only the facade and the C ABI.
//   constrained_driver <galerkin|rescaled> <iterations> <in> <out>
// in: int32 W, H, C, then int32 presence flags of gx, gy, f, values, wx, wy, lambda, then the present arrays in that
// order (float32; gx, gy, f, values H x W x C interleaved, the weights H x W), then the mask (u8 H x W, non-zero = fixed).
// out: the H x W x C u8 result.  Exit 2 on a throw.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ccp/photomontage.h"

int main(int argc, char **argv)
{
    if (argc != 5) return 1;
    const std::string kind = argv[1];
    const int iterations = std::stoi(argv[2]);
    std::ifstream in(argv[3], std::ios::binary);
    int32_t head[10];
    in.read(reinterpret_cast<char *>(head), sizeof(head));
    const int W = head[0], H = head[1], C = head[2];
    std::vector<float> arr[7];
    ccp::ImageView views[7];
    const ccp::ImageView *ptr[7] = {};
    for (int i = 0; i < 7; ++i) {
        if (!head[3 + i]) continue;
        const int ch = i < 4 ? C : 1;
        arr[i].resize((size_t)W * H * ch);
        in.read(reinterpret_cast<char *>(arr[i].data()), (std::streamsize)(arr[i].size() * sizeof(float)));
        views[i] = ccp::ImageView{arr[i].data(), H, W, ch, (size_t)W * ch * sizeof(float)};
        ptr[i] = &views[i];
    }
    std::vector<uint8_t> mask((size_t)W * H);
    in.read(reinterpret_cast<char *>(mask.data()), (std::streamsize)mask.size());
    const ccp::ImageView mv{mask.data(), H, W, 1, (size_t)W};
    std::vector<uint8_t> out((size_t)W * H * C);
    ccp::ImageView ov{out.data(), H, W, C, (size_t)W * C};
    try {
        ccp::SolveConstrained(ptr[0], ptr[1], ptr[2], ptr[3], mv, ptr[4], ptr[5], ptr[6], ov, iterations, 0,
                              kind == "galerkin" ? ccp::Hierarchy::Galerkin : ccp::Hierarchy::Rescaled);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
    return 0;
}
