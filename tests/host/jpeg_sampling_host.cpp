// jpeg_sampling_host.cpp -- the device's two entropy decoders (salve_amd/csrc/jpeg_entropy.h, jpeg_entropy_lanes.h) in the samplings
// beyond 4:2:0, compiled for the HOST from the very same headers as a stand-alone program, so that AddressSanitizer and UBSan judge
// what they do with well-formed and malformed scans (tests/test_jpeg_sampling_host.py builds it with -fsanitize=address,undefined
// -fno-sanitize-recover=all and runs it as a child process).
//
//   jpeg_sampling_host IN OUT
// IN:  int32 cases; per case: int32 sampling (JE_SAMPLING_*), uint8 huffman[4][272], int32 mcus, int32 nbytes, int32 nseg,
//      nseg x {int64 offset, int32 bytes, int32 image, int32 first_mcu, int32 mcu_count}, the nbytes of the scan buffer.
// OUT: per case: uint32 status of the lanes decoder (the OR over the segments; a segment outside the buffer or the image: JE_BAD_SLOT,
//      nothing decoded), uint32 status of the serial decoder over the same segments, int32 rounds of pass B, uint32 1 if the serial
//      decoder left the very same coefficients (else 0), int16 coef[mcus][blocks of an MCU][64] of the lanes decoder (natural order).
// Every segment is decoded from a heap block of its own of exactly bytes + 16 bytes (the padding the library asks its caller for), and
// the coefficients into blocks of exactly their size: a read or write outside either ends the program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../salve_amd/csrc/jpeg_entropy_lanes.h"

static bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

template <int S>
static void run_case(JlShared& sh, JeShared& serial, const JeTables& tab, const std::vector<JlSegment>& segs, const uint8_t* buf, int32_t nbytes, int32_t mcus,
                     FILE* out) {
    constexpr size_t per = JeSampling<S>::coefs;
    std::vector<int16_t> coef((size_t)mcus * per, (int16_t)0), coef_serial((size_t)mcus * per, (int16_t)0);
    uint32_t status = 0, serial_status = 0;
    int32_t rounds = 0;
    je_prepare_tables(sh, tab, 0, 1);
    je_prepare(serial, tab, 0, 1);
    for (const JlSegment& s : segs) {
        if (s.image != 0 || !jl_segment_inside(s, (uint64_t)nbytes + 16, mcus)) {
            status |= JE_BAD_SLOT;
            serial_status |= JE_BAD_SLOT;
            continue;
        }
        uint8_t* scan = (uint8_t*)malloc((size_t)s.bytes + 16);
        if (!scan) exit(2);
        memcpy(scan, buf + s.offset, (size_t)s.bytes);
        memset(scan + s.bytes, 0xA5, 16);
        status |= jl_decode_segment<S>(sh, scan, s.bytes, s.mcu_count, coef.data() + (size_t)s.first_mcu * per, &rounds);
        serial_status |= je_decode_image<S>(serial, scan, s.bytes, s.mcu_count, coef_serial.data() + (size_t)s.first_mcu * per, 0, 1);
        free(scan);
    }
    const uint32_t same = memcmp(coef.data(), coef_serial.data(), coef.size() * sizeof(int16_t)) == 0;
    fwrite(&status, 4, 1, out);
    fwrite(&serial_status, 4, 1, out);
    fwrite(&rounds, 4, 1, out);
    fwrite(&same, 4, 1, out);
    fwrite(coef.data(), 2, coef.size(), out);
}

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
    JlShared* sh = new JlShared();
    JeShared* serial = new JeShared();
    for (int32_t c = 0; c < cases; c++) {
        uint8_t huffman[4 * JE_TABLE_BYTES];
        int32_t sampling = 0, mcus = 0, nbytes = 0, nseg = 0;
        if (!read_all(in, &sampling, 4) || !read_all(in, huffman, sizeof huffman) || !read_all(in, &mcus, 4) || !read_all(in, &nbytes, 4) || !read_all(in, &nseg, 4)) return 2;
        if (mcus < 0 || nbytes < 0 || nseg < 0) return 2;
        std::vector<JlSegment> segs((size_t)nseg);
        if (!read_all(in, segs.data(), segs.size() * sizeof(JlSegment))) return 2;
        uint8_t* buf = (uint8_t*)malloc((size_t)nbytes + 16);
        if (!buf || !read_all(in, buf, (size_t)nbytes)) return 2;
        memset(buf + nbytes, 0xA5, 16);
        JeTables tab;
        if (!je_make_tables(huffman, &tab)) {
            fprintf(stderr, "case %d: the tables are refused\n", c);
            return 3;
        }
        switch (sampling) {
            case JE_SAMPLING_420: run_case<JE_SAMPLING_420>(*sh, *serial, tab, segs, buf, nbytes, mcus, out); break;
            case JE_SAMPLING_422: run_case<JE_SAMPLING_422>(*sh, *serial, tab, segs, buf, nbytes, mcus, out); break;
            case JE_SAMPLING_444: run_case<JE_SAMPLING_444>(*sh, *serial, tab, segs, buf, nbytes, mcus, out); break;
            case JE_SAMPLING_GREY: run_case<JE_SAMPLING_GREY>(*sh, *serial, tab, segs, buf, nbytes, mcus, out); break;
            default: fprintf(stderr, "case %d: sampling %d\n", c, sampling); return 2;
        }
        free(buf);
    }
    delete sh;
    delete serial;
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
