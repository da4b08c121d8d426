// Stand-alone host program over the native loader (tf_kaldi_speaker_amd/csrc/xv_loader.cpp, compiled INTO this program by
// tests/test_loader_sanitized.py, once with the address + undefined-behaviour instrumentation and once with the thread one).
//
//   loader_san <scenario> <work dir> [<data dir>]
//
// scenarios: codec | hostile | create_leaks | stream (stream needs the Kaldi data directory that tests/kaldi_fixture.py writes).
// Every failed expectation prints one "FAILED [scenario] ..." line; the exit status is non-zero if there was any.  The instrumented
// runtime reports on its own (and ends the program) when the loader touches memory it must not, overflows a signed integer or races.
#include "xvector_io.h"

#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

static int g_failed = 0, g_checks = 0;
static const char* g_scenario = "";

static void failed(const char* fmt, ...) {
    ++g_failed;
    fprintf(stderr, "FAILED [%s] ", g_scenario);
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
#define EXPECT(cond, ...) do { ++g_checks; if (!(cond)) failed(__VA_ARGS__); } while (0)

// rc != 0 and the message holds `fragment` and names `file`
static void expect_refused(int rc, const std::string& msg, const char* fragment, const std::string& file, const std::string& what) {
    EXPECT(rc != 0, "%s: accepted (expected \"%s\")", what.c_str(), fragment);
    if (rc == 0) return;
    EXPECT(msg.find(fragment) != std::string::npos, "%s: message \"%s\" lacks \"%s\"", what.c_str(), msg.c_str(), fragment);
    EXPECT(msg.find(file) != std::string::npos, "%s: message \"%s\" does not name %s", what.c_str(), msg.c_str(), file.c_str());
}

// ---------------------------------------------------------------------------------------------------------------------------------
// files
// ---------------------------------------------------------------------------------------------------------------------------------
static void write_file(const std::string& path, const std::string& data) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(data.data(), 1, data.size(), f) != data.size()) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}
static void make_dir(const std::string& path) {
    if (mkdir(path.c_str(), 0777) != 0 && access(path.c_str(), W_OK) != 0) { fprintf(stderr, "cannot create %s\n", path.c_str()); exit(2); }
}
static void put32(std::string& s, int32_t v) { s.append((const char*)&v, 4); }
static void putf(std::string& s, float v) { s.append((const char*)&v, 4); }

// "\0B" + "FM " / "DM " + \4 rows \4 cols
static std::string plain_header(char kind, int32_t rows, int32_t cols) {
    std::string s("\0B", 2);
    s += kind; s += "M "; s += '\4'; put32(s, rows); s += '\4'; put32(s, cols);
    return s;
}
// "\0B" + "CM " + min, range, rows, cols
static std::string cm_header(float minv, float range, int32_t rows, int32_t cols) {
    std::string s("\0BCM ", 5);
    putf(s, minv); putf(s, range); put32(s, rows); put32(s, cols);
    return s;
}

struct Lcg {
    uint64_t x;
    uint32_t next() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(x >> 33); }
};

// the 'CM ' codec in float, as compressed-matrix.h states it (this program is compiled without contraction, like the loader)
static float cm_value(float minv, float range, const uint16_t h[4], uint8_t b) {
    const float gs = range * 1.52590218966964e-05f;
    const float p0 = minv + gs * (float)h[0], p25 = minv + gs * (float)h[1], p75 = minv + gs * (float)h[2], p100 = minv + gs * (float)h[3];
    if (b <= 64) return p0 + (p25 - p0) / 64.0f * (float)b;
    if (b <= 192) return p25 + (p75 - p25) / 128.0f * ((float)b - 64.0f);
    return p75 + (p100 - p75) / 63.0f * ((float)b - 192.0f);
}

struct Mat {
    char kind;
    int rows, cols;
    std::string blob;            // the matrix as it stands in an ark, from its "\0B"
    size_t header_bytes;         // marker, kind, shape (and the column headers of 'CM ')
    std::vector<float> want;     // [rows][cols] as the loader must deliver it
};

static Mat make_mat(char kind, int rows, int cols, uint64_t seed) {
    Mat m;
    m.kind = kind; m.rows = rows; m.cols = cols;
    m.want.resize((size_t)rows * cols);
    Lcg g{seed * 977 + (uint64_t)kind};
    if (kind == 'C') {
        const float minv = -3.5f, range = 11.25f;
        m.blob = cm_header(minv, range, rows, cols);
        std::vector<uint16_t> h((size_t)cols * 4);
        for (int c = 0; c < cols; ++c) {
            uint32_t v = g.next() % 9000;
            for (int k = 0; k < 4; ++k) { h[c * 4 + k] = (uint16_t)v; v += 1 + g.next() % 14000; }
        }
        m.blob.append((const char*)h.data(), h.size() * 2);
        m.header_bytes = m.blob.size();
        static const uint8_t edges[] = {0, 64, 65, 192, 193, 255};
        for (int c = 0; c < cols; ++c)
            for (int r = 0; r < rows; ++r) {
                const uint32_t v = g.next();
                const uint8_t b = (v & 3) == 0 ? edges[(v >> 8) % 6] : (uint8_t)(v >> 8);
                m.blob += (char)b;
                m.want[(size_t)r * cols + c] = cm_value(minv, range, &h[c * 4], b);
            }
    } else {
        m.blob = plain_header(kind, rows, cols);
        m.header_bytes = m.blob.size();
        for (size_t i = 0; i < m.want.size(); ++i) {
            if (kind == 'F') {
                const float v = ((float)(g.next() % 20001) - 10000.0f) / 7.0f;
                putf(m.blob, v);
                m.want[i] = v;
            } else {
                const double v = ((double)(g.next() % 20001) - 10000.0) / 7.0;      // not a float: the loader rounds it
                m.blob.append((const char*)&v, 8);
                m.want[i] = (float)v;
            }
        }
    }
    return m;
}

// one speaker "s1" with the listed "utt rxspecifier frames" triples
struct UttLine { std::string utt, rx; int frames; };
static void write_dir(const std::string& dir, const std::vector<UttLine>& utts) {
    make_dir(dir);
    std::string scp, s2u = "s1", nf;
    for (const UttLine& u : utts) {
        scp += u.utt + " " + u.rx + "\n";
        s2u += " " + u.utt;
        nf += u.utt + " " + std::to_string(u.frames) + "\n";
    }
    write_file(dir + "/feats.scp", scp);
    write_file(dir + "/spk2utt", s2u + "\n");
    write_file(dir + "/utt2num_frames", nf);
    write_file(dir + "/spklist", "s1 0\n");
}

static void set_mmap(bool on) {
    if (on) unsetenv("XVIO_NO_MMAP");
    else setenv("XVIO_NO_MMAP", "1", 1);        // read when an ark is opened
}

// ---------------------------------------------------------------------------------------------------------------------------------
// codec
// ---------------------------------------------------------------------------------------------------------------------------------
static const uint32_t kCanary = 0x7fc0dead;

static void codec_case(const Mat& m, const std::string& path, int start, int length) {
    const int64_t len = length < 0 ? (int64_t)m.rows - start : (int64_t)length;
    const bool in_range = start >= 0 && len >= 0 && (int64_t)start + len <= m.rows;
    const int64_t need = in_range ? len * m.cols : 0;
    const int64_t caps[3] = {need, need - 1, 0};
    for (int k = 0; k < 3; ++k) {
        const int64_t cap = caps[k];
        char what[256];
        snprintf(what, sizeof(what), "%cM %dx%d start %d length %d capacity %lld", m.kind, m.rows, m.cols, start, length, (long long)cap);
        // the buffer ends 64 floats after what the call may write: a stray store inside shows in the canary, one beyond it in the runtime
        std::vector<uint32_t> buf((size_t)need + 64, kCanary);
        int32_t rows = -7, cols = -7;
        const int rc = xvio_read_rows(path.c_str(), 4, start, length, (float*)buf.data(), cap, &rows, &cols);
        const std::string msg = xvio_last_error();
        size_t intact_from = 0;
        if (!in_range) expect_refused(rc, msg, "The number of frames is not enough", path, what);
        else if (cap < need) expect_refused(rc, msg, "output buffer too small", path, what);
        else {
            EXPECT(rc == 0, "%s: refused: %s", what, msg.c_str());
            if (rc != 0) continue;
            EXPECT(rows == len && cols == m.cols, "%s: delivered %d x %d", what, rows, cols);
            const bool same = need == 0 || memcmp(buf.data(), m.want.data() + (size_t)start * m.cols, (size_t)need * 4) == 0;
            EXPECT(same, "%s: the rows differ from the matrix written", what);
            intact_from = (size_t)need;
        }
        bool intact = true;
        for (size_t i = intact_from; i < buf.size(); ++i) intact = intact && buf[i] == kCanary;
        EXPECT(intact, "%s: wrote past %zu floats", what, intact_from);
    }
}

static void scenario_codec(const std::string& work) {
    static const int shapes[][2] = {{1, 1}, {2, 1}, {1, 24}, {2, 24}, {37, 1}, {37, 24}};
    int n = 0;
    for (char kind : {'C', 'F', 'D'})
        for (const auto& sh : shapes) {
            const Mat m = make_mat(kind, sh[0], sh[1], (uint64_t)++n);
            const std::string path = work + "/codec_" + std::to_string(n) + ".ark";
            write_file(path, "key " + m.blob);
            const int R = m.rows;
            const int cases[][2] = {{0, R}, {R - 1, 1}, {R, 0}, {R, -1}, {0, -1}, {R / 2, -1}, {0, -2}, {R / 2, R - R / 2}, {0, 0},
                                    {-1, 1}, {-1, -1}, {-1, 0}, {INT32_MIN, 1}, {INT32_MIN, -1}, {R + 1, -1}, {R + 5, -1}, {R + 1, 0},
                                    {0, R + 1}, {1, R}, {R, 1}, {R - 1, 2}, {INT32_MAX, 1}, {INT32_MAX, INT32_MAX}, {INT32_MAX, -1},
                                    {0, INT32_MAX}, {1, INT32_MAX}};
            for (const auto& c : cases) codec_case(m, path, c[0], c[1]);
        }
    float x[4];
    int32_t r, c;
    const std::string missing = work + "/missing.ark";
    int rc = xvio_read_rows(missing.c_str(), 0, 0, -1, x, 4, &r, &c);
    expect_refused(rc, xvio_last_error(), "cannot open", missing, "a missing ark");
    rc = xvio_read_rows(nullptr, 0, 0, -1, x, 4, &r, &c);
    EXPECT(rc != 0 && strstr(xvio_last_error(), "null argument"), "null path: %d \"%s\"", rc, xvio_last_error());
    rc = xvio_read_rows(missing.c_str(), 0, 0, -1, nullptr, 4, &r, &c);
    EXPECT(rc != 0 && strstr(xvio_last_error(), "null argument"), "null out: %d \"%s\"", rc, xvio_last_error());
    rc = xvio_read_rows(missing.c_str(), 0, 0, -1, x, 4, nullptr, &c);
    EXPECT(rc != 0 && strstr(xvio_last_error(), "null argument"), "null rows: %d \"%s\"", rc, xvio_last_error());
}

// ---------------------------------------------------------------------------------------------------------------------------------
// hostile
// ---------------------------------------------------------------------------------------------------------------------------------
struct LoaderTrial {
    int frames = 10;             // what utt2num_frames claims
    int T = 4;                   // min_len = max_len
    int segments = 1;
    bool packed = false;
};

// create + one next on `dir`: true when either was refused (msg = its message); a loader without a dimension is a failure of its own
static bool loader_refuses(const std::string& dir, const LoaderTrial& t, bool mapped, std::string& msg, const std::string& what) {
    set_mmap(mapped);
    const std::string spklist = dir + "/spklist";
    xvio_config c{};
    c.data_dir = dir.c_str(); c.spklist = spklist.c_str();
    c.num_speakers = 1; c.num_segments = t.segments; c.min_len = c.max_len = t.T;
    c.shuffle = 0; c.num_threads = 1; c.queue_depth = 1; c.seed = 1; c.packed = t.packed ? 1 : 0;
    xvio_loader* l = nullptr;
    msg.clear();
    if (xvio_loader_create(&c, &l)) {
        msg = xvio_last_error();
        EXPECT(l == nullptr, "%s: a refused create left a loader behind", what.c_str());
        return true;
    }
    const int dim = xvio_loader_dim(l);
    EXPECT(dim > 0, "%s: a loader with dim %d", what.c_str(), dim);
    bool refused = false;
    if (dim > 0) {
        const size_t bytes = t.packed ? (size_t)t.segments * (size_t)xvio_packed_chunk_bytes(dim, t.T) : (size_t)t.segments * t.T * dim * 4;
        std::vector<uint8_t> feats(bytes);
        std::vector<int32_t> labels(t.segments);
        int32_t frames = 0;
        const int rc = t.packed ? xvio_loader_next_packed(l, feats.data(), labels.data(), &frames)
                                : xvio_loader_next(l, (float*)feats.data(), labels.data(), &frames);
        if (rc) { refused = true; msg = xvio_last_error(); }
    }
    xvio_loader_destroy(l);
    return refused;
}

static int g_hostile = 0;

// `content` is the ark (key text included) and `offset` what feats.scp says; rr / ld: the message of xvio_read_rows (whole matrix) and of
// the loader, nullptr = that reader has no part in the entry; `file`: what the message must name (the ark when empty)
static void hostile(const std::string& work, const std::string& name, const std::string& content, long long offset, const char* rr,
                    const char* ld, LoaderTrial t = LoaderTrial(), std::string file = "", const std::string& second_utt_rx = "") {
    const std::string stem = work + "/h" + std::to_string(++g_hostile);
    const std::string ark = stem + ".ark", dir = stem + ".d";
    write_file(ark, content);
    if (file.empty()) file = ark;
    if (rr) {
        std::vector<float> out(1 << 16);
        int32_t rows = 0, cols = 0;
        const int rc = xvio_read_rows(ark.c_str(), offset, 0, -1, out.data(), (int64_t)out.size(), &rows, &cols);
        expect_refused(rc, xvio_last_error(), rr, file, name + " (read_rows)");
    }
    if (ld) {
        std::vector<UttLine> utts{{"s1-u1", ark + ":" + std::to_string(offset), t.frames}};
        if (!second_utt_rx.empty()) utts.push_back({"s1-u2", ark + ":" + second_utt_rx, t.frames});
        write_dir(dir, utts);
        for (int packed = 0; packed <= (t.packed ? 1 : 0); ++packed)
            for (int mapped = 1; mapped >= 0; --mapped) {
                LoaderTrial tt = t;
                tt.packed = packed != 0;
                const std::string what = name + (packed ? " (packed loader, " : " (loader, ") + (mapped ? "mapped)" : "pread)");
                std::string msg;
                const bool refused = loader_refuses(dir, tt, mapped != 0, msg, what);
                expect_refused(refused ? 1 : 0, msg, ld, file, what);
            }
        set_mmap(true);
    }
}

static void scenario_hostile(const std::string& work) {
    const char* bad = "shape", * small = "output buffer too small", * cut = "truncated", * nohead = "cannot read the matrix header";
    char name[128];
    // 'FM ' / 'DM ' shapes; three bytes follow each header, less than one element.  INT32_MAX rows of 5 are a shape a file could have:
    // refused by the caller's capacity, or as truncated
    for (char k : {'F', 'D'}) {
        for (int32_t cols : {-3, -1, 0, INT32_MIN}) {
            snprintf(name, sizeof(name), "%cM rows 10 cols %d", k, cols);
            hostile(work, name, "key " + plain_header(k, 10, cols) + std::string(3, 'x'), 4, bad, bad);
        }
        for (int32_t rows : {-1, 0, INT32_MIN}) {
            snprintf(name, sizeof(name), "%cM rows %d cols 5", k, rows);
            hostile(work, name, "key " + plain_header(k, rows, 5) + std::string(3, 'x'), 4, bad, bad);
        }
        snprintf(name, sizeof(name), "%cM rows 10 cols INT32_MAX", k);
        hostile(work, name, "key " + plain_header(k, 10, INT32_MAX) + std::string(3, 'x'), 4, small, small);
        snprintf(name, sizeof(name), "%cM rows INT32_MAX cols 5", k);
        hostile(work, name, "key " + plain_header(k, INT32_MAX, 5) + std::string(3, 'x'), 4, small, cut);
        // products past 32 bits (2^32, and the first square above 2^31): 64-bit arithmetic holds them, the file does not
        snprintf(name, sizeof(name), "%cM 65536 x 65536", k);
        hostile(work, name, "key " + plain_header(k, 65536, 65536) + std::string(3, 'x'), 4, small, cut);
        snprintf(name, sizeof(name), "%cM 46341 x 46341", k);
        hostile(work, name, "key " + plain_header(k, 46341, 46341) + std::string(3, 'x'), 4, small, cut);
        snprintf(name, sizeof(name), "%cM INT32_MAX x 2", k);
        hostile(work, name, "key " + plain_header(k, INT32_MAX, 2) + std::string(3, 'x'), 4, small, cut);
        // rows * cols * elem past 63 bits
        snprintf(name, sizeof(name), "%cM INT32_MAX x INT32_MAX", k);
        hostile(work, name, "key " + plain_header(k, INT32_MAX, INT32_MAX) + std::string(3, 'x'), 4, bad, bad);
        snprintf(name, sizeof(name), "%cM INT32_MIN x INT32_MIN", k);
        hostile(work, name, "key " + plain_header(k, INT32_MIN, INT32_MIN) + std::string(3, 'x'), 4, bad, bad);
        snprintf(name, sizeof(name), "%cM -1 x -1", k);
        hostile(work, name, "key " + plain_header(k, -1, -1) + std::string(3, 'x'), 4, bad, bad);
    }
    // 'CM ' shapes
    const int32_t cm_bad[][2] = {{0, 5}, {-1, 5}, {5, 0}, {5, -2}, {-4, -4}, {INT32_MIN, 5}, {5, INT32_MIN}, {INT32_MIN, INT32_MIN}};
    for (const auto& s : cm_bad) {
        snprintf(name, sizeof(name), "CM %d x %d", s[0], s[1]);
        hostile(work, name, "key " + cm_header(0.0f, 1.0f, s[0], s[1]) + std::string(96, 'x'), 4, bad, bad);
    }
    hostile(work, "CM rows 10 cols INT32_MAX", "key " + cm_header(0.0f, 1.0f, 10, INT32_MAX) + std::string(96, 'x'), 4, small, small);
    hostile(work, "CM rows INT32_MAX cols 5", "key " + cm_header(0.0f, 1.0f, INT32_MAX, 5) + std::string(96, 'x'), 4, small, cut);
    hostile(work, "CM INT32_MAX x INT32_MAX", "key " + cm_header(0.0f, 1.0f, INT32_MAX, INT32_MAX) + std::string(96, 'x'), 4, small, small);
    // markers and kinds
    const Mat fm = make_mat('F', 6, 5, 1);
    hostile(work, "marker \\0C", "key " + std::string("\0C", 2) + fm.blob.substr(2), 4, "not a binary Kaldi object", "not a binary Kaldi object");
    hostile(work, "marker AB", "key AB" + fm.blob.substr(2), 4, "not a binary Kaldi object", "not a binary Kaldi object");
    hostile(work, "marker B\\0", "key " + std::string("B\0", 2) + fm.blob.substr(2), 4, "not a binary Kaldi object", "not a binary Kaldi object");
    hostile(work, "kind XM", "key " + std::string("\0BXM ", 5) + fm.blob.substr(5), 4, "The header contained 'XM '", "The header contained 'XM '");
    hostile(work, "kind HM", "key " + std::string("\0BHM ", 5) + fm.blob.substr(5), 4, "The header contained 'HM '", "The header contained 'HM '");
    hostile(work, "kind FV", "key " + std::string("\0BFV ", 5) + fm.blob.substr(5), 4, "The header contained 'FV '", "The header contained 'FV '");
    // every truncation from the marker to 16 bytes past the header region, and three lengths inside the data.  A chunk is shorter than
    // its utterance, so the longest the loader reads is rows [0, rows-1) (no shuffle): the three lengths are the middle of the data and
    // one and two bytes short of that read's last byte (row-major: the end of the last row but one; 'CM ', column-major: the last
    // column's last byte but one).  The file short of its very last byte is for xvio_read_rows alone, which reads the whole matrix.
    for (char k : {'C', 'F', 'D'}) {
        const Mat m = make_mat(k, 6, 5, 2);
        const size_t total = m.blob.size(), data = total - m.header_bytes;
        const size_t read_end = k == 'C' ? total - 1 : total - data / m.rows;
        std::vector<size_t> lens;
        for (size_t n = 0; n <= m.header_bytes + 16; ++n) lens.push_back(n);
        lens.push_back(m.header_bytes + 16 + (data - 16) / 2);
        lens.push_back(read_end - 2);
        lens.push_back(read_end - 1);
        LoaderTrial t;
        t.frames = m.rows; t.T = m.rows - 1; t.packed = k == 'C';
        for (size_t n : lens) {
            snprintf(name, sizeof(name), "%cM 6x5 cut after %zu of %zu bytes", k, n, total);
            hostile(work, name, "key " + m.blob.substr(0, n), 4, n < 5 ? nohead : cut, n < 5 ? nohead : cut, t);
        }
        snprintf(name, sizeof(name), "%cM 6x5 without its last byte", k);
        hostile(work, name, "key " + m.blob.substr(0, total - 1), 4, cut, nullptr);
    }
    // feats.scp offsets
    const Mat cm = make_mat('C', 20, 5, 3);
    const std::string good = "key " + cm.blob;
    hostile(work, "offset -1", good, -1, nohead, nohead);
    hostile(work, "offset 0 (the key text)", good, 0, "not a binary Kaldi object", "not a binary Kaldi object");
    hostile(work, "offset = file size", good, (long long)good.size(), nohead, nohead);
    hostile(work, "offset = file size - 1", good, (long long)good.size() - 1, nohead, nohead);
    // utt2num_frames
    LoaderTrial t;
    t.frames = 1000; t.T = 50; t.packed = true;
    hostile(work, "utt2num_frames claims 1000 rows of 20", good, 4, nullptr, "The number of frames is not enough", t);
    t.frames = 21; t.T = 20;
    hostile(work, "utt2num_frames claims 21 rows of 20", good, 4, nullptr, "The number of frames is not enough", t);
    t = LoaderTrial();
    t.frames = 0;
    hostile(work, "utt2num_frames 0", good, 4, nullptr, "has 0 frames", t, "utt2num_frames");
    t.frames = -5;
    hostile(work, "utt2num_frames -5", good, 4, nullptr, "has -5 frames", t, "utt2num_frames");
    // a second utterance with other columns (both utterances of the one speaker are in the batch: two segments of two)
    for (char k : {'C', 'F', 'D'})
        for (int cols2 : {3, 7}) {
            const Mat a = make_mat(k, 30, 5, 4), b = make_mat(k, 30, cols2, 5);
            const std::string two = "u1 " + a.blob + "u2 ";
            LoaderTrial d;
            d.frames = 30; d.T = 10; d.segments = 2; d.packed = k == 'C';
            snprintf(name, sizeof(name), "%cM 5 columns, then %d", k, cols2);
            hostile(work, name, two + b.blob, 3, nullptr, "feature dimension changes", d, "", std::to_string(two.size()));
        }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// create_leaks
// ---------------------------------------------------------------------------------------------------------------------------------
static int count_fds() {
    DIR* d = opendir("/proc/self/fd");
    if (!d) return -1;
    int n = 0;
    while (dirent* e = readdir(d)) if (e->d_name[0] != '.') ++n;
    closedir(d);
    return n;
}
static int count_ark_maps() {
    std::ifstream f("/proc/self/maps");
    std::string line;
    int n = 0;
    while (std::getline(f, line)) if (line.find(".ark") != std::string::npos) ++n;
    return n;
}

struct DirText {               // a file is not written when its text is "-"
    std::string spklist = "s1 0\ns2 1\n", spk2utt = "s1 u1 u2\ns2 u3\n", frames = "u1 80\nu2 80\nu3 80\n", scp;
};

static void scenario_create_leaks(const std::string& work) {
    const std::string a = work + "/a.ark", b = work + "/b.ark", c = work + "/c.ark";
    write_file(a, "key " + make_mat('C', 80, 5, 1).blob);
    write_file(b, "key " + make_mat('C', 80, 5, 2).blob);
    write_file(c, "key " + make_mat('C', 80, 5, 3).blob);
    const std::string two = "u1 " + a + ":4\nu2 " + b + ":4\n";           // two arks are open when the third line is read
    int ndir = 0;
    auto run = [&](const std::string& what, DirText t, const char* fragment, int speakers = 1, int min_len = 20, int max_len = 30) {
        const std::string dir = work + "/leak" + std::to_string(++ndir);
        make_dir(dir);
        if (t.scp.empty()) t.scp = two + "u3 " + c + ":4\n";
        if (t.spklist != "-") write_file(dir + "/spklist", t.spklist);
        if (t.spk2utt != "-") write_file(dir + "/spk2utt", t.spk2utt);
        if (t.frames != "-") write_file(dir + "/utt2num_frames", t.frames);
        if (t.scp != "-") write_file(dir + "/feats.scp", t.scp);
        const std::string spklist = dir + "/spklist";
        for (int mapped = 1; mapped >= 0; --mapped) {
            set_mmap(mapped != 0);
            const std::string w = what + (mapped ? " (mapped)" : " (pread)");
            xvio_config cfg{};
            cfg.data_dir = dir.c_str(); cfg.spklist = spklist.c_str();
            cfg.num_speakers = speakers; cfg.num_segments = 2; cfg.min_len = min_len; cfg.max_len = max_len;
            cfg.shuffle = 1; cfg.num_threads = 2; cfg.queue_depth = 2; cfg.seed = 5;
            const int fds = count_fds(), maps = count_ark_maps();
            xvio_loader* l = nullptr;
            const int rc = xvio_loader_create(&cfg, &l);
            const std::string msg = rc ? xvio_last_error() : "";
            if (fragment) {
                EXPECT(rc != 0 && msg.find(fragment) != std::string::npos, "%s: create gave %d \"%s\", expected \"%s\"", w.c_str(), rc, msg.c_str(), fragment);
                if (rc == 0) xvio_loader_destroy(l);
            } else {
                EXPECT(rc == 0, "%s: create refused: %s", w.c_str(), msg.c_str());
                if (rc == 0) {
                    EXPECT(count_fds() == fds + 3, "%s: %d descriptors while three arks are open, %d before", w.c_str(), count_fds(), fds);
                    EXPECT(count_ark_maps() == maps + (mapped ? 3 : 0), "%s: %d ark mappings, %d before", w.c_str(), count_ark_maps(), maps);
                    std::vector<float> feats((size_t)speakers * 2 * max_len * xvio_loader_dim(l));
                    std::vector<int32_t> labels((size_t)speakers * 2);
                    int32_t frames;
                    for (int i = 0; i < 2; ++i) EXPECT(xvio_loader_next(l, feats.data(), labels.data(), &frames) == 0, "%s: %s", w.c_str(), xvio_last_error());
                    xvio_loader_destroy(l);
                }
            }
            EXPECT(count_fds() == fds, "%s: %d open descriptors before, %d after", w.c_str(), fds, count_fds());
            EXPECT(count_ark_maps() == maps, "%s: %d ark mappings before, %d after", w.c_str(), maps, count_ark_maps());
        }
        set_mmap(true);
    };
    DirText t;
    t = DirText(); t.spklist = "-"; run("missing spklist", t, "cannot open");
    t = DirText(); t.spk2utt = "-"; run("missing spk2utt", t, "cannot open");
    t = DirText(); t.frames = "-"; run("missing utt2num_frames", t, "Expect utt2num_frames exists");
    t = DirText(); t.scp = "-"; run("missing feats.scp", t, "cannot open");
    t = DirText(); t.spk2utt = "s1 u1 u2\ns3 u3\n"; run("speaker not in spklist", t, "speaker s3 of spk2utt is not in");
    t = DirText(); t.scp = two + "u3 no_offset_here\n"; run("third scp line without ':'", t, "is not path:offset");
    t = DirText(); t.spk2utt = "s1 u1 u2\n"; run("third utterance not in spk2utt", t, "utterance u3 of feats.scp is not in spk2utt");
    t = DirText(); t.frames = "u1 80\nu2 80\n"; run("third utterance not in utt2num_frames", t, "utterance u3 of feats.scp is not in utt2num_frames");
    t = DirText(); t.scp = two + "u3 " + work + "/no_such.ark:4\n"; run("third ark cannot be opened", t, "cannot open");
    t = DirText(); t.scp = "\n"; run("empty feats.scp", t, "lists no utterance");
    t = DirText(); t.scp = "u1 " + a + ":5\nu2 " + b + ":4\nu3 " + c + ":4\n"; run("bad first matrix", t, "not a binary Kaldi object");
    t = DirText(); t.frames = "u1 80\nu2 80\nu3 0\n"; run("an utterance of 0 frames", t, "has 0 frames");
    t = DirText(); run("0 speakers per batch", t, "bad batch shape", 0);
    t = DirText(); run("max_len < min_len", t, "bad batch shape", 1, 30, 20);
    t = DirText(); run("min_len 0", t, "bad batch shape", 1, 0, 20);
    t = DirText(); run("a well-formed directory", t, nullptr, 2);
    xvio_loader* l = nullptr;
    EXPECT(xvio_loader_create(nullptr, &l) != 0 && strstr(xvio_last_error(), "null argument"), "null config: \"%s\"", xvio_last_error());
}

// ---------------------------------------------------------------------------------------------------------------------------------
// stream
// ---------------------------------------------------------------------------------------------------------------------------------
static uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

struct StreamCfg {
    int threads = 1, depth = 1, packed = 0, speakers = 5, segments = 3, min_len = 40, max_len = 65;
    uint64_t seed = 11;
};

static xvio_loader* open_stream(const std::string& data, const StreamCfg& s) {
    const std::string spklist = data + "/spklist";
    xvio_config c{};
    c.data_dir = data.c_str(); c.spklist = spklist.c_str();
    c.num_speakers = s.speakers; c.num_segments = s.segments; c.min_len = s.min_len; c.max_len = s.max_len;
    c.shuffle = 1; c.num_threads = s.threads; c.queue_depth = s.depth; c.seed = s.seed; c.packed = s.packed;
    xvio_loader* l = nullptr;
    if (xvio_loader_create(&c, &l)) { failed("create on %s: %s", data.c_str(), xvio_last_error()); return nullptr; }
    return l;
}

struct Batches {
    std::vector<uint64_t> hash;      // 0 for a failed batch
    std::string pattern;             // 'o' / 'x' per batch
    std::string first_error;
};

// the next n batches: frames, labels and EVERY delivered byte (a packed chunk's padding included) go into the hash
static Batches take(xvio_loader* l, const StreamCfg& s, int n) {
    Batches out;
    const int dim = xvio_loader_dim(l);
    const size_t B = (size_t)s.speakers * s.segments;
    const size_t cap = s.packed ? B * (size_t)xvio_packed_chunk_bytes(dim, s.max_len) : B * s.max_len * dim * 4;
    std::vector<uint8_t> feats(cap);
    std::vector<int32_t> labels(B);
    for (int i = 0; i < n; ++i) {
        memset(feats.data(), 0xA5, cap);
        int32_t frames = 0;
        const int rc = s.packed ? xvio_loader_next_packed(l, feats.data(), labels.data(), &frames)
                                : xvio_loader_next(l, (float*)feats.data(), labels.data(), &frames);
        if (rc) {
            if (out.first_error.empty()) out.first_error = xvio_last_error();
            out.hash.push_back(0);
            out.pattern += 'x';
            continue;
        }
        const size_t bytes = s.packed ? B * (size_t)xvio_packed_chunk_bytes(dim, frames) : B * (size_t)frames * dim * 4;
        uint64_t h = fnv(14695981039346656037ull, &frames, 4);
        h = fnv(h, labels.data(), B * 4);
        h = fnv(h, feats.data(), bytes);
        out.hash.push_back(h ? h : 1);
        out.pattern += 'o';
    }
    return out;
}

static Batches run_stream(const std::string& data, const StreamCfg& s, int n) {
    xvio_loader* l = open_stream(data, s);
    if (!l) return Batches();
    Batches b = take(l, s, n);
    xvio_loader_destroy(l);
    return b;
}

static void scenario_stream(const std::string& data) {
    const int N = 24;
    int longest = 0;
    {
        std::ifstream f(data + "/utt2num_frames");
        std::string utt; int n;
        while (f >> utt >> n) longest = n > longest ? n : longest;
    }
    EXPECT(longest > 70, "%s/utt2num_frames: longest utterance %d", data.c_str(), longest);
    Batches ref[2];
    for (int packed = 0; packed < 2; ++packed) {
        // 1. the stream is a function of (seed, index): thread count and ring depth change nothing, down to the last delivered byte
        bool have = false;
        for (int threads : {1, 2, 8})
            for (int depth : {1, 2, 5}) {
                StreamCfg s;
                s.threads = threads; s.depth = depth; s.packed = packed;
                const Batches b = run_stream(data, s, N);
                EXPECT(b.pattern == std::string(N, 'o'), "packed %d threads %d depth %d: batches %s (%s)", packed, threads, depth, b.pattern.c_str(),
                       b.first_error.c_str());
                if (!have) { ref[packed] = b; have = true; continue; }
                for (int i = 0; i < N && i < (int)b.hash.size(); ++i)
                    EXPECT(b.hash[i] == ref[packed].hash[i], "packed %d threads %d depth %d: batch %d differs from threads 1 depth 1", packed, threads, depth, i);
            }
        StreamCfg other;
        other.threads = 2; other.depth = 2; other.packed = packed; other.seed = 12;
        const Batches o = run_stream(data, other, N);
        int same = 0;
        for (int i = 0; i < N && i < (int)o.hash.size(); ++i) same += o.hash[i] == ref[packed].hash[i];
        EXPECT(o.hash.size() == (size_t)N && same == 0, "packed %d: seed 12 repeats %d batches of seed 11", packed, same);

        // 2. lengths on both sides of the longest utterance: a batch whose T no utterance exceeds fails, the others arrive as ever
        StreamCfg edge;
        edge.packed = packed; edge.speakers = 1; edge.segments = 2; edge.min_len = longest - 6; edge.max_len = longest + 5; edge.depth = 3;
        Batches first;
        for (int threads : {1, 2, 8}) {
            edge.threads = threads;
            const Batches b = run_stream(data, edge, N);
            if (threads == 1) {
                first = b;
                const size_t x = b.pattern.find('x');
                EXPECT(x != std::string::npos && b.pattern.find('o', x) != std::string::npos, "packed %d: no batch after a failed one in %s", packed, b.pattern.c_str());
                EXPECT(b.first_error.find("no speaker has an utterance longer than") != std::string::npos, "packed %d: \"%s\"", packed, b.first_error.c_str());
                continue;
            }
            EXPECT(b.pattern == first.pattern, "packed %d threads %d: ok/failed %s, one thread %s", packed, threads, b.pattern.c_str(), first.pattern.c_str());
            EXPECT(b.hash == first.hash, "packed %d threads %d: the batches around failed ones differ from one thread's", packed, threads);
        }

        // 3. destroy while the workers are busy
        StreamCfg busy;
        busy.threads = 8; busy.depth = 5; busy.packed = packed;
        xvio_loader* l = open_stream(data, busy);
        xvio_loader_destroy(l);                                   // directly after create
        l = open_stream(data, busy);
        if (l) {
            const Batches b = take(l, busy, 3);
            EXPECT(b.pattern == "ooo", "packed %d: %s", packed, b.pattern.c_str());
            int64_t done = 0;
            for (int spin = 0; spin < 20000 && done < 3 + busy.depth; ++spin) {      // the ring fills: depth batches past the consumer
                xvio_loader_stats(l, &done, nullptr);
                std::this_thread::sleep_for(std::chrono::microseconds(500));
            }
            EXPECT(done >= 3 + busy.depth, "packed %d: the ring did not fill (%lld batches)", packed, (long long)done);
            xvio_loader_destroy(l);                               // every slot ready, every worker waiting for a free one
        }
        edge.threads = 8;
        l = open_stream(data, edge);
        if (l) {
            Batches b;
            int taken = 0;
            do { b = take(l, edge, 1); } while (b.pattern == "o" && ++taken < 200);
            EXPECT(b.pattern == "x", "packed %d: no failed batch in 200", packed);
            xvio_loader_destroy(l);                               // directly after a failed fetch
        }

        // 4. two loaders alive on the same arks, each consumed by a thread of its own
        StreamCfg twin;
        twin.threads = 2; twin.depth = 2; twin.packed = packed;
        xvio_loader* la = open_stream(data, twin);
        xvio_loader* lb = open_stream(data, twin);
        if (la && lb) {
            Batches ba, bb;
            std::thread ta([&] { ba = take(la, twin, N); });
            std::thread tb([&] { bb = take(lb, twin, N); });
            ta.join(); tb.join();
            EXPECT(ba.hash == ref[packed].hash && bb.hash == ref[packed].hash, "packed %d: two loaders at once deliver other batches than one", packed);
        }
        xvio_loader_destroy(la);
        xvio_loader_destroy(lb);

        // 5. the wrong fetch for the mode, and null arguments
        StreamCfg one;
        one.packed = packed;
        l = open_stream(data, one);
        if (l) {
            std::vector<uint8_t> feats(15 * (size_t)xvio_packed_chunk_bytes(xvio_loader_dim(l), 65) * 4);
            std::vector<int32_t> labels(15);
            int32_t frames;
            const int rc = packed ? xvio_loader_next(l, (float*)feats.data(), labels.data(), &frames)
                                  : xvio_loader_next_packed(l, feats.data(), labels.data(), &frames);
            const char* want = packed ? "created in packed mode" : "decodes on the host";
            EXPECT(rc != 0 && strstr(xvio_last_error(), want), "packed %d, the other mode's fetch: %d \"%s\"", packed, rc, xvio_last_error());
            auto next = [&](xvio_loader* h, void* f, int32_t* lab, int32_t* fr) {
                return packed ? xvio_loader_next_packed(h, (uint8_t*)f, lab, fr) : xvio_loader_next(h, (float*)f, lab, fr);
            };
            EXPECT(next(nullptr, feats.data(), labels.data(), &frames) != 0 && strstr(xvio_last_error(), "null argument"), "null loader: \"%s\"", xvio_last_error());
            EXPECT(next(l, nullptr, labels.data(), &frames) != 0 && strstr(xvio_last_error(), "null argument"), "null features: \"%s\"", xvio_last_error());
            EXPECT(next(l, feats.data(), nullptr, &frames) != 0 && strstr(xvio_last_error(), "null argument"), "null labels: \"%s\"", xvio_last_error());
            EXPECT(next(l, feats.data(), labels.data(), nullptr) != 0 && strstr(xvio_last_error(), "null argument"), "null frames: \"%s\"", xvio_last_error());
            // the refusals consumed nothing: the next batch is batch 0
            const Batches b = take(l, one, 1);
            EXPECT(b.hash.size() == 1 && b.hash[0] == ref[packed].hash[0], "packed %d: batch 0 after refused fetches differs", packed);
            xvio_loader_destroy(l);
        }
    }
    xvio_loader_destroy(nullptr);
    EXPECT(xvio_loader_dim(nullptr) == 0 && xvio_loader_stats(nullptr, nullptr, nullptr) != 0, "null loader queries");
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s codec|hostile|create_leaks|stream <work dir> [<data dir>]\n", argv[0]);
        return 2;
    }
    g_scenario = argv[1];
    const std::string scenario = argv[1], work = argv[2];
    make_dir(work);
    if (scenario == "codec") scenario_codec(work);
    else if (scenario == "hostile") scenario_hostile(work);
    else if (scenario == "create_leaks") scenario_create_leaks(work);
    else if (scenario == "stream" && argc > 3) scenario_stream(argv[3]);
    else { fprintf(stderr, "unknown scenario %s (or stream without a data directory)\n", argv[1]); return 2; }
    printf("%s [%s] %d checks, %d failed\n", g_failed ? "FAILED" : "ok", g_scenario, g_checks, g_failed);
    return g_failed ? 1 : 0;
}
