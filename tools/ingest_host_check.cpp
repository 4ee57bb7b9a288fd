// The host path of the edge-list parser (graphem-rapids_amd/csrc/ingest_core.h) as a stand-alone program, for a run under
// the sanitizers on a CPU:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ingest_host_check.cpp -o ingest_host_check
//     ./ingest_host_check [file ...]
//
// Without arguments it parses the grammar cases of tests/datasets_checks.py and a generated boundary text (lines of 3 to 40
// bytes, CR LF on every 7th, a 10 000-byte comment, a row with 5 000 blanks between its fields), each in every format, mode
// and vertex rule, from a heap buffer of exactly the text's size, so that one byte read past a line's end is an error; it
// also walks the chunk cuts for several chunk sizes and checks that they fall after whole terminators and cover the text.
// With arguments it parses those files (format by suffix).  Exit status 0: everything ran and the invariants held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../graphem-rapids_amd/csrc/ingest_core.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// every format, mode and vertex rule; returns the data rows of the snap reading (-1: a bad line)
static int64_t run(const std::string &text, int only_format = -1) {
    const int64_t n = (int64_t)text.size();
    std::unique_ptr<uint8_t[]> heap(new uint8_t[(size_t)n]);          // exactly n bytes: no slack behind the text
    std::memcpy(heap.get(), text.data(), (size_t)n);
    const uint8_t *t = heap.get();
    int64_t snap_rows = -1;
    for (int format = 0; format < 3; ++format) {
        if (only_format >= 0 && format != only_format) continue;
        const int64_t off = ingest_data_offset(t, n, format);
        CHECK(off >= 0 && off <= n);
        std::vector<int64_t> rows;
        const int64_t bad = ingest_host_rows(t, n, off, format, &rows);
        if (bad >= 0) {
            const std::string msg = ingest_error_text(t, n, bad, format);
            CHECK(msg.compare(0, 5, "line ") == 0);
            continue;
        }
        if (format == GH_INGEST_SNAP) snap_rows = (int64_t)rows.size() / 2;
        for (int directed = 0; directed < 2; ++directed)
            for (int from_rows = 0; from_rows < 2; ++from_rows) {
                ingest_result res;
                std::string err;
                CHECK(ingest_host_finish(std::vector<int64_t>(rows), directed != 0, from_rows != 0, &res, &err) == GH_OK);
                CHECK(res.R == (int64_t)rows.size() / 2 && res.E <= res.R);
                CHECK(std::is_sorted(res.vertices.begin(), res.vertices.end()));
                for (int relabel = 0; relabel < 2; ++relabel) {
                    std::vector<int64_t> out(2 * (size_t)res.E);
                    ingest_host_edges(res, relabel != 0, out.data());
                    for (int64_t e = 0; e < res.E; ++e) {
                        if (!directed) CHECK(out[2 * e] < out[2 * e + 1]);
                        if (relabel) CHECK(out[2 * e] >= 0 && out[2 * e + 1] < (int64_t)res.vertices.size());
                    }
                }
            }
        for (int64_t chunk : {1, 7, 16, 100, 4096}) {
            int64_t pos = off, count = 0;
            while (pos < n) {
                const int64_t end = ingest_chunk_end(t, n, pos, chunk);
                CHECK(end > pos && end <= n);
                if (end < n) CHECK(t[end - 1] == '\n' || (t[end - 1] == '\r' && t[end] != '\n'));
                pos = end;
                ++count;
            }
            CHECK(pos == n || n <= off);
            (void)count;
        }
    }
    return snap_rows;
}

static std::string boundary_text() {
    std::string s;
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int i = 0; i < 200000; ++i) {
        std::string line = std::to_string(next() % 1000000007ull % (uint64_t)std::max<int64_t>(10, (int64_t)(next() % 1000000000))) + " " +
                           std::to_string(next() % (1ull << (1 + next() % 30)));
        const size_t pad = next() % 20;
        if (pad && line.size() + pad + 1 <= 38) line += std::string(pad, ' ') + "w";
        if (i == 70001) line = "#" + std::string(9999, 'c');
        if (i == 130003) line = "123" + std::string(2500, ' ') + std::string(2500, '\t') + "456";
        s += line + (i % 7 == 0 ? "\r\n" : "\n");
    }
    return s;
}

int main(int argc, char **argv) {
    if (argc > 1) {
        for (int a = 1; a < argc; ++a) {
            std::FILE *f = std::fopen(argv[a], "rb");
            if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
            std::string text;
            char buf[1 << 16];
            for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
            std::fclose(f);
            const std::string name = argv[a];
            const auto ends = [&](const char *suffix) { const size_t k = std::strlen(suffix); return name.size() >= k && name.compare(name.size() - k, k, suffix) == 0; };
            const int format = ends(".mtx") ? GH_INGEST_MTX : ends(".edges") ? GH_INGEST_EDGES : GH_INGEST_SNAP;
            std::printf("%s: %lld bytes, format %d\n", argv[a], (long long)text.size(), format);
            run(text, format);
        }
        return failures ? 1 : 0;
    }
    const std::vector<std::string> grammar = {
        "1 2\n3 4", "1 2\r\n3 4\r\n", "1 2\r3 4\r", "1 2\n3 4\r\n5 6\r7 8\n\r9 10\r\r\n11 12", "\n\n1 2\n\n\n3 4\n\n", "\r\n\r\n1 2\r\n\r\n",
        "  \t1 2 \t \n\t3\t4\t\n", "+7 -3\n007 0000000000000000000000012\n-0 +0\n",
        "9223372036854775807 -9223372036854775808\n-9223372036854775808 0\n", "1 2 zzz\n3 4 0.5 1e-3\n5 6 1_0 \xd9\xa3\n",
        "1 2\nxyz\n3 4\n#\n-\n", "# a\n#1 2\n1 2\n# b c d\n3 4\n#last 5 6", "1 2\n \t \n3 4\n", "", "# x\n# y 1 2\n", "\n\r\n\r\r\n", "4 9\n", "4 9",
        "5 3\n3 5\n5 3\n4 4\n3 9\n9 9\n", "1 1\n2 2\n1 1\n", "\r", "\n", " ", "1", "-", "1 ", " 1 2", "1 2\r",
        // errors
        "1 2\n # x y\n", "1 2\n3 4\n1 2x\n", "1_0 2\n", "9223372036854775808 1", "1 2\n3 -9223372036854775809", "5 6\n- 1\n", "1 2\n\xd9\xa3 4\n",
        "%%MM\n3 3 2\n1 2\n% a b\n2 3\n", "%h\n1 1 1\n-9223372036854775808 5\n", "1 2\nx y\n3 4\nz w\n", "1 2\r\n3 4\r\n\r\n5 q\r\n6 7\r\n", "+", "+ -",
        "99999999999999999999999999999999999999 1x", "%", "%\r", "%\r\n", "%a\n\n1 2\n", "%%MatrixMarket\r\n% c\r\n3 3 2\r\n1 2\r\n2 3 0.5\r\n"};
    for (const std::string &text : grammar) run(text);
    for (int c : {0x09, 0x0B, 0x0C, 0x1C, 0x1D, 0x1E, 0x1F, 0x20}) {
        const std::string b(1, (char)c);
        CHECK(run("5" + b + "6\n" + b + "7" + b + b + "8" + b + "\n") == 2);
    }
    for (int c : {0x00, 0x08, 0x1B, 0x21, 0x7F, 0x80, 0x85, 0xA0, 0xFF}) CHECK(run("5" + std::string(1, (char)c) + "6 7\n") == -1);
    CHECK(run("1 2\n3 4") == 2 && run("") == 0 && run("1 2 zzz\n3 4 0.5 1e-3\n5 6 1_0 \xd9\xa3\n") == 3 && run("1_0 2\n") == -1);
    const std::string big = boundary_text();
    CHECK(run(big) == 199999);
    std::printf("ingest host check: %zu grammar texts, boundary text of %zu bytes, %d failures\n", grammar.size(), big.size(), failures);
    return failures ? 1 : 0;
}
