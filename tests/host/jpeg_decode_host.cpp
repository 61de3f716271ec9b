// jpeg_decode_host.cpp -- the device's entropy decoder (salve_amd/csrc/jpeg_entropy.h), compiled for the HOST from the very same
// header as a stand-alone program, so that AddressSanitizer and UBSan judge what it does with malformed scans
// (tests/test_jpeg_decode_host.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it as a child process).
//
//   jpeg_decode_host IN OUT
// IN:  int32 cases; per case: uint8 huffman[4][272], int32 mcus, int32 nbytes, the scan's bytes.
// OUT: per case: uint32 status, int16 coef[mcus][6][64] (natural order).
// Every scan is decoded from a heap block of its own of exactly nbytes + 16 bytes (the padding the library asks its caller for), and
// the coefficients into a block of exactly their size: a read or write outside either ends the program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../salve_amd/csrc/jpeg_entropy.h"

static bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open the files\n");
        return 2;
    }
    int32_t cases = 0;
    if (!read_all(in, &cases, 4) || cases < 0) return 2;
    JeShared* sh = new JeShared();
    for (int32_t c = 0; c < cases; c++) {
        uint8_t huffman[4 * JE_TABLE_BYTES];
        int32_t mcus = 0, nbytes = 0;
        if (!read_all(in, huffman, sizeof huffman) || !read_all(in, &mcus, 4) || !read_all(in, &nbytes, 4) || mcus < 0 || nbytes < 0) return 2;
        uint8_t* scan = (uint8_t*)malloc((size_t)nbytes + 16);
        if (!scan || !read_all(in, scan, (size_t)nbytes)) return 2;
        memset(scan + nbytes, 0xA5, 16);
        JeTables tab;
        if (!je_make_tables(huffman, &tab)) {
            fprintf(stderr, "case %d: the tables are refused\n", c);
            return 3;
        }
        std::vector<int16_t> coef((size_t)mcus * 384, (int16_t)0x5A5A);
        je_prepare(*sh, tab, 0, 1);
        const uint32_t status = je_decode_image(*sh, scan, nbytes, mcus, coef.data(), 0, 1);
        fwrite(&status, 4, 1, out);
        fwrite(coef.data(), 2, coef.size(), out);
        free(scan);
    }
    delete sh;
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
