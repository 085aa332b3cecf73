// hog_math_check.cpp -- compv_amd/csrc/hog_math.hpp run on the host (standard library only, no GPU): the whole HOG of ONE frame, cell after cell and
// block after block in the order the kernels of hog_kernels.hip take, so that tests/test_hog_host.py can hold the header's arithmetic against
// tests/hog_model.py and the golden descriptors bit for bit.  Built with -fsanitize=address,undefined: every index below is checked while it runs.
//   in:  int32 W, H, blockW, blockH, strideW, strideH, cellW, cellH, nbins, norm, gradient, interp (resolved: no zero field),
//              cellsX, cellsY, validX, validY, blocksX, blocksY, cpbX, cpbY, stepX, stepY; uint8 gray[H][W]
//   out: float32 cells[cellsY][cellsX][nbins]; float32 desc[blocksY * blocksX][cpbY * cpbX * nbins]
// Build with -ffp-contract=off (one rounding per operation).
#include "../../compv_amd/csrc/hog_math.hpp"

#include <cstdio>
#include <vector>

using namespace compvhip::hog;

namespace {
struct Header {
	int32_t W, H, blockW, blockH, strideW, strideH, cellW, cellH, nbins, norm, gradient, interp;
	int32_t cellsX, cellsY, validX, validY, blocksX, blocksY, cpbX, cpbY, stepX, stepY;
};
struct Hist {
	float* h;
	float& operator[](int b) { return h[b]; }
};

template <int INTERP>
void cell(const Header& q, const std::vector<uint8_t>& gray, int cx, int cy, float* h)
{
	const Binning bin = binning(q.nbins, q.gradient == 1);
	Hist hist{h};
	for (int j = 0; j < q.cellH; ++j) {
		for (int i = 0; i < q.cellW; ++i) {
			const int x = cx * q.strideW + i, y = cy * q.strideH + j;
			const bool xb = x == 0 || x == q.W - 1, yb = y == 0 || y == q.H - 1;
			// a neighbour outside the frame is never used (the border rule): read the pixel itself in its place
			const int left = gray.at(static_cast<size_t>(y) * q.W + (xb ? x : x - 1)), right = gray.at(static_cast<size_t>(y) * q.W + (xb ? x : x + 1));
			const int up = gray.at(static_cast<size_t>(yb ? y : y - 1) * q.W + x), down = gray.at(static_cast<size_t>(yb ? y : y + 1) * q.W + x);
			float gx, gy;
			gradient(left, right, up, down, xb, yb, gx, gy);
			vote<INTERP>(hist, bin, magnitude(gx, gy), direction(gx, gy));
		}
	}
}
} // namespace

int main(int argc, char** argv)
{
	if (argc != 3) { fprintf(stderr, "usage: hog_math_check in.bin out.bin\n"); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	Header q;
	if (fread(&q, sizeof(q), 1, f) != 1) return 2;
	std::vector<uint8_t> gray(static_cast<size_t>(q.W) * q.H);
	if (fread(gray.data(), 1, gray.size(), f) != gray.size()) return 2;
	fclose(f);

	std::vector<float> cells(static_cast<size_t>(q.cellsY) * q.cellsX * q.nbins, 0.f);          // the left-out cells stay 0
	for (int cy = 0; cy < q.validY; ++cy) {
		for (int cx = 0; cx < q.validX; ++cx) {
			float* h = &cells[(static_cast<size_t>(cy) * q.cellsX + cx) * q.nbins];
			if (q.interp == kInterpNearest) cell<kInterpNearest>(q, gray, cx, cy, h);
			else cell<kInterpBilinear>(q, gray, cx, cy, h);
		}
	}
	const int count = q.cpbY * q.cpbX * q.nbins;
	std::vector<float> desc(static_cast<size_t>(q.blocksY) * q.blocksX * count);
	for (int by = 0; by < q.blocksY; ++by) {
		for (int bx = 0; bx < q.blocksX; ++bx) {
			const BlockLoad v{&cells[(static_cast<size_t>(by) * q.stepY * q.cellsX + static_cast<size_t>(bx) * q.stepX) * q.nbins], q.cpbX * q.nbins, q.cellsX * q.nbins};
			// every element the block gathers lies in the map
			if ((by * q.stepY + q.cpbY) > q.cellsY || (bx * q.stepX + q.cpbX) > q.cellsX) { fprintf(stderr, "block (%d, %d) leaves the map\n", bx, by); return 1; }
			normalize_block(v, count, q.norm, &desc[(static_cast<size_t>(by) * q.blocksX + bx) * count]);
		}
	}
	f = fopen(argv[2], "wb");
	if (!f) return 2;
	if (fwrite(cells.data(), sizeof(float), cells.size(), f) != cells.size() || fwrite(desc.data(), sizeof(float), desc.size(), f) != desc.size()) return 2;
	fclose(f);
	return 0;
}
