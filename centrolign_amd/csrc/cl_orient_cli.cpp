// cl_orient_cli.cpp — centrolign-orient: the layer in front of centrolign that its reference asks its users to build themselves ("it does not
// identify inversions ... you will need to build additional layers around centrolign to generate global, non-inverting alignment problems").
// Host code over the C ABI only: cl_parse_fasta, cl_strand_profile_compute on the first device of --devices, cl_strand_intervals, cl_strand_apply
// and the two TSV writers.  The intervals go to standard output; --profile and --fasta-out name the other two results.
// Conventions of the main tool: every failure is "error: <message>" and status 1; output files must not exist yet; what is wrong with the
// command line is said before the FASTA is read or a device opened.
#include <errno.h>
#include <getopt.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "centrolign_amd.h"

namespace {

const long long kMaxWindow = 1 << 20, kMaxText = 1ll << 30;

int fail(const std::string& msg) {
    fprintf(stderr, "error: %s\n", msg.c_str());
    return 1;
}

std::string lib_error(const cl_context* ctx = nullptr) {
    const char* e = cl_last_error(ctx);
    if (!e || !*e) e = cl_last_error(nullptr);
    return e && *e ? e : "unknown error";
}

void print_help() {
    cl_strands_params d;
    cl_strands_params_default(&d);
    fprintf(stderr, "Usage: centrolign-orient [options] sequences.fasta   ('-' reads standard input)\n\n");
    fprintf(stderr, "Finds the inverted intervals and the flipped sequences of a set of sequences from the strands of their own k-mers and writes them as a table\n");
    fprintf(stderr, "to standard output: sample start end length windows forward reverse whole (0-based, half-open).\n\n");
    fprintf(stderr, "Options:\n");
    fprintf(stderr, " -k INT                     k-mer length, 1 to 31 [%d]\n", d.k);
    fprintf(stderr, " --window / -w INT          Window in bases, 1 to %lld [%u]\n", kMaxWindow, d.window);
    fprintf(stderr, " --min-run INT              Least length of a run of reverse windows that is reported, in windows [1]\n");
    fprintf(stderr, " --profile FILE             Write kmers, forward, reverse, neutral and the call of every window to FILE (which must not exist yet)\n");
    fprintf(stderr, " --fasta-out FILE           Write the sequences with the intervals turned back to FILE (which must not exist yet): the input for centrolign\n");
    fprintf(stderr, " --devices LIST             Comma-separated device ordinals; the first one is used [0]\n");
    fprintf(stderr, " -v INT                     Verbosity; at 3 the windows, distinct k-mers, intervals and device times are logged [0]\n");
    fprintf(stderr, " -h                         Print this message and exit\n");
}

// a whole number from least to most, digits alone
bool parse_whole(const std::string& text, long long least, long long most, long long& out) {
    if (text.empty() || text.size() > 18 || text.find_first_not_of("0123456789") != std::string::npos) return false;
    const long long v = strtoll(text.c_str(), nullptr, 10);
    if (v < least || v > most) return false;
    out = v;
    return true;
}

bool parse_devices(const std::string& s, std::vector<int>& out) {
    size_t pos = 0;
    while (pos <= s.size()) {
        size_t comma = s.find(',', pos);
        if (comma == std::string::npos) comma = s.size();
        long long v = 0;
        if (!parse_whole(s.substr(pos, comma - pos), 0, 1 << 20, v)) return false;
        out.push_back((int)v);
        pos = comma + 1;
    }
    return !out.empty();
}

bool read_input(const std::string& name, std::string& out, std::string& err) {
    FILE* f = name == "-" ? stdin : fopen(name.c_str(), "rb");
    if (!f) { err = "Could not open file " + name; return false; }
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, n);
    const bool ok = !ferror(f);
    if (f != stdin) fclose(f);
    if (!ok) err = "Could not read file " + name;
    return ok;
}

bool write_file(const std::string& to, const char* text, size_t len) {
    FILE* f = fopen(to.c_str(), "wb");
    const bool written = f && fwrite(text, 1, len, f) == len;
    return !((f && fclose(f) != 0) || !written);
}

std::string expects(const char* option, const std::string& what, const char* text) { return std::string(option) + " expects " + what + ", got '" + text + "'"; }

// what the run holds of the library's, released on every way out
struct Held {
    cl_fasta fa;
    bool parsed = false;
    cl_context* ctx = nullptr;
    cl_strand_profile profile;
    cl_strand_interval* intervals = nullptr;
    char *profile_tsv = nullptr, *intervals_tsv = nullptr;
    Held() { memset(&profile, 0, sizeof(profile)); }
    Held(const Held&) = delete;
    Held& operator=(const Held&) = delete;
    ~Held() {
        free(profile_tsv);
        free(intervals_tsv);
        cl_strand_intervals_free(intervals);
        cl_strand_profile_free(&profile);
        if (ctx) cl_context_destroy(ctx);
        if (parsed) cl_fasta_free(&fa);
    }
};

int run(int argc, char** argv) {
    cl_strands_params params;
    cl_strands_params_default(&params);
    long long min_run = 1, verbosity = 0, v = 0;
    std::string profile_file, fasta_out;
    std::vector<int> devices;
    enum { OPT_MIN_RUN = 1000, OPT_PROFILE, OPT_FASTA_OUT, OPT_DEVICES };
    static const option LONG[] = {{"window", required_argument, nullptr, 'w'},          {"min-run", required_argument, nullptr, OPT_MIN_RUN},
                                  {"profile", required_argument, nullptr, OPT_PROFILE}, {"fasta-out", required_argument, nullptr, OPT_FASTA_OUT},
                                  {"devices", required_argument, nullptr, OPT_DEVICES}, {nullptr, 0, nullptr, 0}};
    opterr = 0;
    for (int c; (c = getopt_long(argc, argv, ":k:w:v:h", LONG, nullptr)) != -1;) {
        switch (c) {
        case 'k':
            if (!parse_whole(optarg, 1, 31, v)) return fail(expects("-k", "a whole number from 1 to 31", optarg));
            params.k = (int32_t)v;
            break;
        case 'w':
            if (!parse_whole(optarg, 1, kMaxWindow, v)) return fail(expects("--window", "a whole number from 1 to " + std::to_string(kMaxWindow), optarg));
            params.window = (uint32_t)v;
            break;
        case OPT_MIN_RUN:
            if (!parse_whole(optarg, 1, 0xFFFFFFFFll, min_run)) return fail(expects("--min-run", "a whole number from 1 to 4294967295", optarg));
            break;
        case 'v':
            if (!parse_whole(optarg, 0, 1000, verbosity)) return fail(expects("-v", "a whole number", optarg));
            break;
        case OPT_PROFILE: profile_file = optarg; break;
        case OPT_FASTA_OUT: fasta_out = optarg; break;
        case OPT_DEVICES:
            devices.clear();
            if (!parse_devices(optarg, devices)) return fail(expects("--devices", "comma-separated device ordinals", optarg));
            break;
        case 'h': print_help(); return 0;
        case ':': return fail(std::string("option ") + argv[optind - 1] + " needs a value");
        default: return fail(std::string("unknown option ") + argv[optind - 1]);
        }
    }
    if (argc - optind != 1) return fail(argc == optind ? "no FASTA file was given (-h shows the options)" : "more than one FASTA file was given");
    const std::string input = argv[optind];
    if (!profile_file.empty() && profile_file == fasta_out) return fail("--profile and --fasta-out name the same file");
    if (!profile_file.empty() && std::ifstream(profile_file).good()) return fail("--profile file already exists: " + profile_file);
    if (!fasta_out.empty() && std::ifstream(fasta_out).good()) return fail("--fasta-out file already exists: " + fasta_out);

    Held h;
    std::string text, err;
    if (!read_input(input, text, err)) return fail(err);
    if (cl_parse_fasta(nullptr, text.data(), text.size(), &h.fa)) return fail(lib_error());
    h.parsed = true;
    const cl_fasta& fa = h.fa;
    const uint64_t n = fa.n_sequences;
    unsigned long long total = 0;
    for (uint64_t i = 0; i < n; ++i)
        if ((total += fa.lengths[i]) >= (unsigned long long)kMaxText) return fail("the sequences hold 2^30 bases or more (at " + std::string(fa.names[i]) + ")");
    std::vector<std::string> shown;   // as --pair-stats of centrolign names them
    for (uint64_t i = 0; i < n; ++i) {
        shown.emplace_back(fa.names[i]);
        std::replace(shown.back().begin(), shown.back().end(), '/', '_');
    }
    std::vector<const char*> names;
    for (const std::string& nm : shown) names.push_back(nm.c_str());

    h.ctx = cl_context_create(devices.empty() ? 0 : devices[0]);
    if (!h.ctx) return fail("no usable GPU: " + lib_error());
    if (cl_strand_profile_compute(h.ctx, fa.sequences, fa.lengths, n, &params, &h.profile)) return fail("the strand profile: " + lib_error(h.ctx));
    uint64_t n_intervals = 0, len = 0;
    if (cl_strand_intervals(&h.profile, (uint32_t)min_run, &h.intervals, &n_intervals)) return fail("the intervals: " + lib_error());
    if (verbosity >= 3)
        fprintf(stderr, "[orient] %llu sequences, %llu bases, %llu windows, %llu distinct k-mers, %llu intervals; sort %.3f ms, votes %.3f ms\n", (unsigned long long)n,
                (unsigned long long)h.profile.n_bases, (unsigned long long)h.profile.n_windows, (unsigned long long)h.profile.distinct, (unsigned long long)n_intervals,
                h.profile.sort_ms, h.profile.vote_ms);
    if (!profile_file.empty()) {
        if (cl_strand_profile_tsv(&h.profile, names.data(), &h.profile_tsv, &len)) return fail("the profile: " + lib_error());
        if (!write_file(profile_file, h.profile_tsv, len)) return fail("could not write the profile to " + profile_file);
    }
    if (!fasta_out.empty()) {
        std::string out;
        for (uint64_t i = 0; i < n; ++i) {
            std::string turned(fa.lengths[i], '\0');
            if (cl_strand_apply(fa.sequences[i], fa.lengths[i], i, h.intervals, n_intervals, &turned[0])) return fail("the sequences: " + lib_error());
            out += ">" + std::string(fa.names[i]) + "\n" + turned + "\n";
        }
        if (!write_file(fasta_out, out.data(), out.size())) return fail("could not write the sequences to " + fasta_out);
    }
    if (cl_strand_intervals_tsv(h.intervals, n_intervals, names.data(), n, &h.intervals_tsv, &len)) return fail("the intervals: " + lib_error());
    if (fwrite(h.intervals_tsv, 1, len, stdout) != len || fflush(stdout) != 0) return fail("could not write the intervals to standard output");
    return 0;
}

}  // namespace

int main(int argc, char** argv) { return run(argc, argv); }
