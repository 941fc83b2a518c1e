// Host-only driver of the region blend facade (include/ccp/photomontage.h: ccp::BlendRegion, ccp::SeamlessClone),
// built by tests/test_gpu_region_blend.py and tests/test_blend_facade.py with the g++ line of tests/cpp/Makefile.
//
// usage: blend_driver <field|import|mixed> <gs|cg|lex|mg> <iterations> <in.bin> <out.bin>
//   in.bin: int32 W, H, C; mask H*W u8; then for `field` gx, gy (H*W*C float32 each) and canvas (H*W*C u8), else
//   source and target (H*W*C u8 each).  out.bin: the H*W*C u8 composite, written only when the call returned.
// Any exception: its message on stderr, exit status 2, no output file.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "ccp/photomontage.h"

int main(int argc, char **argv)
{
    if (argc != 6) {
        std::cerr << "usage: blend_driver <field|import|mixed> <gs|cg|lex|mg> <iterations> <in.bin> <out.bin>\n";
        return 1;
    }
    const std::string mode = argv[1], solver_name = argv[2];
    const int iterations = std::atoi(argv[3]);
    std::ifstream in(argv[4], std::ios::binary);
    std::vector<char> blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (blob.size() < 12) {
        std::cerr << "short input\n";
        return 1;
    }
    int32_t dims[3];
    std::memcpy(dims, blob.data(), sizeof dims);
    const int W = dims[0], H = dims[1], C = dims[2];
    const std::size_t px = (std::size_t)W * H, n = px * C;
    const std::size_t need = 12 + px + (mode == "field" ? 2 * n * sizeof(float) + n : 2 * n);
    if (blob.size() != need) {
        std::cerr << "input size " << blob.size() << ", expected " << need << "\n";
        return 1;
    }
    char *p = blob.data() + 12;
    const ccp::ImageView mask{p, H, W, 1, (std::size_t)W};
    p += px;
    ccp::Solver solver = ccp::Solver::GaussSeidel;
    if (solver_name == "cg") solver = ccp::Solver::ConjugateGradient;
    else if (solver_name == "lex") solver = ccp::Solver::GaussSeidelReferenceOrder;
    else if (solver_name == "mg") solver = ccp::Solver::MultigridConjugateGradient;
    std::vector<uint8_t> result(n, 0);
    ccp::ImageView out{result.data(), H, W, C, (std::size_t)W * C};
    try {
        if (mode == "field") {
            const ccp::ImageView gx{p, H, W, C, (std::size_t)W * C * sizeof(float)};
            const ccp::ImageView gy{p + n * sizeof(float), H, W, C, (std::size_t)W * C * sizeof(float)};
            const ccp::ImageView canvas{p + 2 * n * sizeof(float), H, W, C, (std::size_t)W * C};
            ccp::BlendRegion(gx, gy, canvas, mask, out, iterations, solver);
        } else {
            const ccp::ImageView source{p, H, W, C, (std::size_t)W * C};
            const ccp::ImageView target{p + n, H, W, C, (std::size_t)W * C};
            ccp::SeamlessClone(source, target, mask, out, mode == "mixed" ? ccp::CloneMode::Mixed : ccp::CloneMode::Import,
                               iterations, solver);
        }
    } catch (const std::exception &e) {
        std::cerr << "error: " << e.what() << "\n";
        return 2;
    }
    std::ofstream(argv[5], std::ios::binary).write(reinterpret_cast<const char *>(result.data()), (std::streamsize)n);
    std::cout << "ok\n";
    return 0;
}
