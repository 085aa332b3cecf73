// moments_math_check.cpp -- compv_amd/csrc/moments_math.hpp on the host: a stand-alone program (standard library only, no GPU) that
// tests/test_moments_host.py builds with AddressSanitizer and UBSan and feeds the records of tests/golden/golden_moments.npz.
//
//   moments_math_check IN OUT
// IN:  int32 n, nsizes; n x 6 uint64 raw records; nsizes x { int32 W, H, weights }.
// OUT: n x compvhip_moments_shape (72 bytes each); nsizes x int32, moments::fits of every size.
// Every shape record is worked out twice, into memory that held 0x00 and 0xff, and the program aborts when the two differ in a byte (a field the
// function left alone would show).
#include "../../compv_amd/csrc/moments_math.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace compvhip;

static void die(const char* what)
{
	fprintf(stderr, "moments_math_check: %s\n", what);
	exit(2);
}

int main(int argc, char** argv)
{
	static_assert(sizeof(compvhip_moments) == 48 && sizeof(compvhip_moments_shape) == 72, "the records of include/compv_hip.h");
	if (argc != 3) die("usage: moments_math_check IN OUT");
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out) die("cannot open a file");
	int32_t h[2];
	if (fread(h, 4, 2, in) != 2 || h[0] < 0 || h[1] < 0) die("bad header");
	std::vector<compvhip_moments> raw(static_cast<size_t>(h[0]));
	std::vector<int32_t> sizes(3 * static_cast<size_t>(h[1]));
	if (!raw.empty() && fread(raw.data(), sizeof(compvhip_moments), raw.size(), in) != raw.size()) die("short input");
	if (!sizes.empty() && fread(sizes.data(), 4, sizes.size(), in) != sizes.size()) die("short input");
	fclose(in);
	for (const compvhip_moments& r : raw) {
		compvhip_moments_shape a, b;
		memset(&a, 0x00, sizeof(a)); memset(&b, 0xff, sizeof(b));
		moments::shape(r, &a); moments::shape(r, &b);
		if (memcmp(&a, &b, sizeof(a))) die("a shape record depends on what its memory held");
		if (fwrite(&a, sizeof(a), 1, out) != 1) die("short output");
	}
	for (size_t k = 0; k < sizes.size(); k += 3) {
		const int32_t ok = moments::fits(static_cast<uint64_t>(static_cast<uint32_t>(sizes[k])), static_cast<uint64_t>(static_cast<uint32_t>(sizes[k + 1])), sizes[k + 2]) ? 1 : 0;
		if (fwrite(&ok, 4, 1, out) != 1) die("short output");
	}
	if (fclose(out)) die("close");
	return 0;
}
