// cl_cli.cpp — the `centrolign` executable: the reference's command line (src/main.cpp) over the library's C ABI.  Options and their
// order of effect are the reference's; the parameters live in a cl_config (cl_config_api.cpp) and the run is one cl_msa call.
// An option is one row of TABLE below and, unless it sets a cl_config parameter, one field of Options: the getopt arrays, the help and
// the --X-only rule are made from the rows.  To add an option, add its row there (and its field), then use the field in the stage that
// needs it; run() at the end of the file is the list of stages.
// Deliberate differences from the reference (also in print_help and README.md):
//   - every failure is "error: <message>" on stderr and exit status 1 (the reference lets some exceptions escape and aborts);
//   - -p takes a decimal number (the reference stores an integer into a Double parameter, which its type check refuses: it aborts);
//   - -t N runs N worker contexts; --devices LIST places them (cl_msa_params.devices);
//   - --infer-tree infers the guide tree from k-mer distances (cl_infer_guide_tree) where the reference needs one from outside; --tree-out
//     writes it;
//   - --refine-tree N rebuilds the guide tree from the distances of an alignment made under it (cl_refine_guide_tree), up to N times, before the
//     alignment proper; --pair-stats and --dist-out write the pairwise statistics and distances the final alignment implies;
//   - --pair-profile (with --window) and --pair-events (with --min-event) write, for every pair of sequences, the induced alignment's columns per
//     window of the first sequence and its long insertions and deletions with their positions (cl_induced_pairwise_profiles,
//     cl_induced_gap_events_batch on the printed graph); not with -c, whose final graph has cycles;
//   - --compare-to GFA with --pair-agreement FILE writes, for every pair of sequences, how many aligned base pairs the printed graph shares with a
//     baseline graph of the same sequences (cl_induced_pairwise_agreements); --graph GFA compares a graph that is already there instead of aligning;
//   - --msa-out, --column-stats and --variable-sites write the alignment as columns: aligned FASTA, a record per column, and the aligned FASTA of
//     the variable sites alone (cl_msa_columns_compute on the printed graph; --msa-layout, --site-min-minor, --site-max-gaps); not with -c;
//   - --dotplot FILE writes the windowed k-mer identity map of the input sequences (cl_kmer_dotplot_compute; --dotplot-k, --dotplot-window,
//     --dotplot-min-identity, --dotplot-pairs) before the alignment starts; --dotplot-only ends the run there;
//   - --periods FILE writes the repeat period spectra of the input sequences (cl_period_spectrum_compute; --periods-hist and the --periods-*
//     options) before the alignment starts; --periods-only ends the run there;
//   - --monomers FILE with --monomers-templates FASTA writes which monomer stands where on every input sequence (cl_monomer_decompose_compute;
//     --monomers-summary and the --monomers-* options) before the alignment starts; --monomers-only ends the run there;
//   - --monomers-rounds N refines the templates first (cl_monomer_templates_refine_compute), --monomers-seed-period cuts them from the first
//     sequence instead of reading them, --monomers-write-templates and --monomers-pileup write the final templates and the per-column counts
//     under them (cl_monomer_pileup_compute);
//   - -v gates this tool's own progress lines; the device is opened only when the alignment starts.
#include <getopt.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "centrolign_amd.h"

namespace {

enum { LOG_SILENT = 0, LOG_MINIMAL = 1, LOG_BASIC = 2, LOG_VERBOSE = 3, LOG_DEBUG = 4 };
int g_level = LOG_BASIC;

void log_line(int level, const std::string& msg) {
    if (level <= g_level) fprintf(stderr, "[centrolign] %s\n", msg.c_str());
}

std::string lib_error() {
    const char* e = cl_last_error(nullptr);
    return e && *e ? e : "unknown error";
}

// what the context reported last, or failing that the library; under a heading ("the dot plot: ...") "failed" stands in instead
std::string context_error(cl_context* ctx, const char* heading = nullptr) {
    const char* e = cl_last_error(ctx);
    if (!heading) return e && *e ? e : lib_error();
    return std::string(heading) + ": " + (e && *e ? e : "failed");
}

int fail(const std::string& msg) {
    fprintf(stderr, "error: %s\n", msg.c_str());
    return 1;
}

// text the library allocated
struct LibText {
    char* text = nullptr;
    uint64_t len = 0;
    LibText() = default;
    LibText(const LibText&) = delete;
    LibText& operator=(const LibText&) = delete;
    ~LibText() { free(text); }
    std::string str() const { return std::string(text, len); }
};

std::string config_value(const cl_config* cfg, const char* name) {
    LibText t;
    return cl_config_get(cfg, name, &t.text) ? std::string() : std::string(t.text);
}

std::string generate(const cl_config* cfg) {
    LibText t;
    return cl_config_generate(cfg, &t.text, &t.len) ? std::string() : t.str();
}

// the whole of a file, or of standard input for "-"
bool read_input(const std::string& name, std::string& out, std::string& err) {
    FILE* f = name == "-" ? stdin : fopen(name.c_str(), "rb");
    if (!f) {
        err = "Could not open file " + name;
        return false;
    }
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, n);
    const bool ok = !ferror(f);
    if (f != stdin) fclose(f);
    if (!ok) err = "Could not read file " + name;
    return ok;
}

// text -> the file, or "could not write <what> to <file>" (what may be empty)
bool write_file(const std::string& to, const char* text, uint64_t len, const std::string& what, std::string& err) {
    FILE* f = fopen(to.c_str(), "wb");
    const bool written = f && fwrite(text, 1, len, f) == len;
    if ((f && fclose(f) != 0) || !written) {
        err = "could not write " + what + (what.empty() ? "to " : " to ") + to;
        return false;
    }
    return true;
}

bool write_file(const std::string& to, const std::string& text, const std::string& what, std::string& err) { return write_file(to, text.data(), text.size(), what, err); }

// "<label> file already exists: <file>" for a named file that is there
bool already_exists(const char* label, const std::string& file, std::string& err) {
    if (file.empty() || !std::ifstream(file).good()) return false;
    err = std::string(label) + " file already exists: " + file;
    return true;
}

// one of a group's own files named again among the files it is compared with: the group's message
bool clashes(const std::vector<std::string>& own, const std::vector<std::string>& others, const std::string& message, std::string& err) {
    for (const std::string& file : own)
        if (!file.empty() && std::find(others.begin(), others.end(), file) != others.end()) {
            err = message;
            return true;
        }
    return false;
}

// a whole number from least to most.  Digits alone, 18 at the most, unless as_strtol: then whatever strtol takes (blanks, a sign)
bool parse_whole(const std::string& text, long long least, long long most, bool as_strtol, long long& out) {
    if (text.empty()) return false;
    if (!as_strtol && (text.size() > 18 || text.find_first_not_of("0123456789") != std::string::npos)) return false;
    char* end = nullptr;
    errno = 0;
    const long long v = strtoll(text.c_str(), &end, 10);
    if (*end || errno || v < least || v > most) return false;
    out = v;
    return true;
}

bool parse_devices(const char* text, std::vector<int>& out) {
    std::string s(text);
    size_t pos = 0;
    while (pos <= s.size()) {
        size_t comma = s.find(',', pos);
        if (comma == std::string::npos) comma = s.size();
        long long v = 0;
        if (!parse_whole(s.substr(pos, comma - pos), 0, 1 << 20, true, v)) return false;
        out.push_back((int)v);
        pos = comma + 1;
    }
    return !out.empty();
}

std::string flat_name(std::string name) {   // a sequence's name as -A names its files
    std::replace(name.begin(), name.end(), '/', '_');
    return name;
}

// ---- the options ------------------------------------------------------------------------------------------------------------------------

// an option as it stood on the command line.  File names that are empty count as not given, as they always have: those are asked with empty()
struct Given {
    std::string text;
    bool given = false;
    bool empty() const { return text.empty(); }
};

enum Group { GROUP_NONE, GROUP_DOTPLOT, GROUP_PERIODS, GROUP_MONOMERS, N_GROUPS };

// the options that set no cl_config parameter
struct Options {
    Given config, generate_config, help, force_gfa_output, devices;
    Given infer_tree, refine_tree, tree_out, pair_stats, dist_out;
    Given pair_profile, window, pair_events, min_event;
    Given compare_to, pair_agreement, graph;
    Given msa_out, column_stats, variable_sites, msa_layout, site_min_minor, site_max_gaps;
    Given dotplot, dotplot_k, dotplot_window, dotplot_min_identity, dotplot_pairs, dotplot_only;
    Given periods, periods_hist, periods_k, periods_window, periods_max, periods_peaks, periods_radius, periods_min_period, periods_min_count, periods_scope, periods_only;
    Given monomers, monomers_templates, monomers_summary, monomers_strands, monomers_match, monomers_mismatch, monomers_insertion, monomers_deletion, monomers_chunk,
        monomers_overlap, monomers_only, monomers_rounds, monomers_write_templates, monomers_pileup, monomers_least_share, monomers_seed_period, monomers_seed_count,
        monomers_seed_start;
    bool beside_only[N_GROUPS] = {};   // an option was given that --<group>-only does not go with
};

struct Opt {
    const char* name;     // --name
    char letter;          // -l, or 0
    const char* meta;     // its argument in the help, or nullptr for a flag
    const char* help;
    bool shows_default;   // the help ends with param's default in brackets
    bool reference;       // the reference tool has it
    Group group;
    const char* param;    // the cl_config parameter it sets, to its argument or to fixed
    const char* fixed;
    Given Options::* into;   // or the field it fills
};
const bool REF = true, ADDED = false;
const char* const NO = nullptr;

// Every option, in the order of the help.  getopt_long's id of a row is its index + ID_BASE.
const Opt TABLE[] = {
    {"tree", 'T', "FILE", "Newick guide tree over the FASTA's sequence names [the sequences in FASTA order]", false, REF, GROUP_NONE, "tree_name", NO, nullptr},
    {"all-pairs", 'A', "PREFIX", "Write the induced alignment of every pair of sequences to files starting with PREFIX", false, REF, GROUP_NONE, "all_pairs_prefix", NO, nullptr},
    {"all-subprobs", 'S', "PREFIX", "Write the alignment of every subtree to files starting with PREFIX", false, REF, GROUP_NONE, "subproblems_prefix", NO, nullptr},
    {"subalignments", 's', "FILE", "Write the aligned paths of every subproblem to FILE (which must not exist yet)", false, REF, GROUP_NONE, "subalignments_filepath", NO, nullptr},
    {"cyclize", 'c', NO, "Merge long tandem duplications into cycles of the final graph", false, REF, GROUP_NONE, "cyclize_tandem_duplications", "true", nullptr},
    {"cyclizing-size", 'y', "INT", "With -c, merge tandem duplications longer than INT bases", true, REF, GROUP_NONE, "min_cyclizing_length", NO, nullptr},
    {"max-count", 'm', "INT", "Use an anchor only if it occurs at most INT times", true, REF, GROUP_NONE, "max_count", NO, nullptr},
    {"max-anchors", 'a', "INT", "Consider at most INT anchors per merge", true, REF, GROUP_NONE, "max_num_match_pairs", NO, nullptr},
    {"count-power", 'p', "FLOAT", "Divide anchor weights by the count raised to FLOAT", true, REF, GROUP_NONE, "pair_count_power", NO, nullptr},
    {"chain-alg", 'g', "INT", "Chaining algorithm: 1 (sparse), 2 (sparse affine)", true, REF, GROUP_NONE, "chaining_algorithm", NO, nullptr},
    {"no-unaln", 'u', NO, "Do not look for unalignable regions", false, REF, GROUP_NONE, "constraint_method", "0", nullptr},
    {"verbosity", 'v', "INT", "0 (silent), 1 (minimal), 2 (basic), 3 (verbose), 4 (debug)", true, REF, GROUP_NONE, "logging_level", NO, nullptr},
    {"config", 'C', "FILE", "Take every parameter from this config file (overrides all other command line input)", false, REF, GROUP_NONE, NO, NO, &Options::config},
    {"generate-config", 'G', NO, "Write a config file with the current parameters to standard output and exit", false, REF, GROUP_NONE, NO, NO, &Options::generate_config},
    {"restart", 'R', NO, "Resume an interrupted run (the first run needs -S)", false, REF, GROUP_NONE, "restart", "true", nullptr},
    {"threads", 't', "INT", "Worker contexts that run calibrations and independent merges side by side", true, REF, GROUP_NONE, "threads", NO, nullptr},
    {"skip-calibration", 0, NO, "Keep the starting score scale instead of calibrating it to the input", false, REF, GROUP_NONE, "skip_calibration", "true", nullptr},
    {"force-gfa-output", 0, NO, "Write a GFA even for two sequences", false, REF, GROUP_NONE, NO, NO, &Options::force_gfa_output},
    {"bond-prefix", 0, "PREFIX", "With -c, write the alignment of every tandem duplication found to files starting with PREFIX", false, REF, GROUP_NONE, "bonds_prefix", NO, nullptr},
    {"devices", 0, "LIST", "Comma-separated GPU ordinals the worker contexts are spread over [the first GPU]", false, ADDED, GROUP_NONE, NO, NO, &Options::devices},
    {"infer-tree", 0, NO, "Infer the guide tree from k-mer distances (k = 21, neighbor joining) instead of taking one", false, ADDED, GROUP_NONE, NO, NO, &Options::infer_tree},
    {"refine-tree", 0, "INT", "Rebuild the guide tree from the distances of an alignment made under it, up to INT times, then align", false, ADDED, GROUP_NONE, NO, NO, &Options::refine_tree},
    {"tree-out", 0, "FILE", "With --infer-tree or --refine-tree, write the Newick tree the alignment used to FILE", false, ADDED, GROUP_NONE, NO, NO, &Options::tree_out},
    {"pair-stats", 0, "FILE", "Write matches, mismatches, gap bases, runs and distance of every pair of sequences to FILE (which must not exist yet)", false, ADDED, GROUP_NONE, NO, NO, &Options::pair_stats},
    {"dist-out", 0, "FILE", "Write the matrix of pairwise alignment distances, in FASTA order, to FILE", false, ADDED, GROUP_NONE, NO, NO, &Options::dist_out},
    {"pair-profile", 0, "FILE", "Write matches, mismatches and gap bases of every pair of sequences per window of the first one to FILE (which must not exist yet; not with -c)", false, ADDED, GROUP_NONE, NO, NO, &Options::pair_profile},
    {"window", 0, "INT", "With --pair-profile, the window in bases of the first sequence [1000]", false, ADDED, GROUP_NONE, NO, NO, &Options::window},
    {"pair-events", 0, "FILE", "Write every insertion and deletion of at least --min-event bases between two sequences, with its positions, to FILE (which must not exist yet; not with -c)", false, ADDED, GROUP_NONE, NO, NO, &Options::pair_events},
    {"min-event", 0, "INT", "With --pair-events, the least length of an insertion or deletion that is written [50]", false, ADDED, GROUP_NONE, NO, NO, &Options::min_event},
    {"compare-to", 0, "GFA", "With --pair-agreement, the baseline graph of the same sequences: an earlier run's, the reference's, a truth graph", false, ADDED, GROUP_NONE, NO, NO, &Options::compare_to},
    {"pair-agreement", 0, "FILE", "Write the aligned base pairs of every pair of sequences here, in the baseline and in both, to FILE (which must not exist yet; not with -c)", false, ADDED, GROUP_NONE, NO, NO, &Options::pair_agreement},
    {"graph", 0, "GFA", "With --compare-to and --pair-agreement, compare GFA as the graph this run would have printed: nothing is aligned or printed", false, ADDED, GROUP_NONE, NO, NO, &Options::graph},
    {"msa-out", 0, "FILE", "Write the alignment as aligned FASTA, one row per sequence, to FILE (which must not exist yet; not with -c)", false, ADDED, GROUP_NONE, NO, NO, &Options::msa_out},
    {"column-stats", 0, "FILE", "Write the base and gap counts, the consensus and the site flag of every alignment column to FILE (which must not exist yet; not with -c)", false, ADDED, GROUP_NONE, NO, NO, &Options::column_stats},
    {"variable-sites", 0, "FILE", "Write the aligned FASTA of the variable sites alone, the site = 1 columns of --column-stats, to FILE (which must not exist yet; not with -c)", false, ADDED, GROUP_NONE, NO, NO, &Options::variable_sites},
    {"msa-layout", 0, "WORD", "With the three above, the columns: level (compact, bubble branches side by side) or node (one graph node per column) [level]", false, ADDED, GROUP_NONE, NO, NO, &Options::msa_layout},
    {"site-min-minor", 0, "INT", "A column is a variable site if its second most frequent base occurs at least INT times [1]", false, ADDED, GROUP_NONE, NO, NO, &Options::site_min_minor},
    {"site-max-gaps", 0, "INT", "... and it has at most INT gaps [no limit]", false, ADDED, GROUP_NONE, NO, NO, &Options::site_max_gaps},
    {"dotplot", 0, "FILE", "Write the windowed k-mer identity map (dot plot) of the input sequences, one row per kept window pair, to FILE (which must not exist yet)", false, ADDED, GROUP_DOTPLOT, NO, NO, &Options::dotplot},
    {"dotplot-k", 0, "INT", "With --dotplot, the k-mer length, 1 to 31 [21]", false, ADDED, GROUP_DOTPLOT, NO, NO, &Options::dotplot_k},
    {"dotplot-window", 0, "INT", "With --dotplot, the window in bases, k to 1048576 [2000]", false, ADDED, GROUP_DOTPLOT, NO, NO, &Options::dotplot_window},
    {"dotplot-min-identity", 0, "FLOAT", "With --dotplot, keep a window pair from this identity in percent on [86]", false, ADDED, GROUP_DOTPLOT, NO, NO, &Options::dotplot_min_identity},
    {"dotplot-pairs", 0, "all|self", "With --dotplot, compare all windows or only the windows of the same sequence [all]", false, ADDED, GROUP_DOTPLOT, NO, NO, &Options::dotplot_pairs},
    {"dotplot-only", 0, NO, "With --dotplot, end after writing the map: nothing is aligned or printed", false, ADDED, GROUP_DOTPLOT, NO, NO, &Options::dotplot_only},
    {"periods", 0, "FILE", "Write the repeat period spectra of the input sequences, one row per peak of every sequence and window, to FILE (which must not exist yet)", false, ADDED, GROUP_PERIODS, NO, NO, &Options::periods},
    {"periods-hist", 0, "FILE", "With --periods, write the non-zero bins of every spectrum to FILE (which must not exist yet)", false, ADDED, GROUP_PERIODS, NO, NO, &Options::periods_hist},
    {"periods-k", 0, "INT", "With --periods, the k-mer length, 1 to 31 [8]", false, ADDED, GROUP_PERIODS, NO, NO, &Options::periods_k},
    {"periods-window", 0, "INT", "With --periods, the window in bases, 1 to 1048576 [10000]", false, ADDED, GROUP_PERIODS, NO, NO, &Options::periods_window},
    {"periods-max", 0, "INT", "With --periods, the longest period counted, 1 to 16383 [8000]", false, ADDED, GROUP_PERIODS, NO, NO, &Options::periods_max},
    {"periods-peaks", 0, "INT", "With --periods, the peaks written per row, 1 to 16 [3]", false, ADDED, GROUP_PERIODS, NO, NO, &Options::periods_peaks},
    {"periods-radius", 0, "INT", "With --periods, a peak is the largest count within INT bins on either side, 1 to 64 [1]", false, ADDED, GROUP_PERIODS, NO, NO, &Options::periods_radius},
    {"periods-min-period", 0, "INT", "With --periods, the shortest period that can be a peak [1]", false, ADDED, GROUP_PERIODS, NO, NO, &Options::periods_min_period},
    {"periods-min-count", 0, "INT", "With --periods, the least count of a peak [2]", false, ADDED, GROUP_PERIODS, NO, NO, &Options::periods_min_count},
    {"periods-scope", 0, "WORD", "With --periods, the rows written: both, sequences or windows [both]", false, ADDED, GROUP_PERIODS, NO, NO, &Options::periods_scope},
    {"periods-only", 0, NO, "With --periods, end after writing the spectra: nothing is aligned or printed", false, ADDED, GROUP_PERIODS, NO, NO, &Options::periods_only},
    {"monomers", 0, "FILE", "Write which monomer of --monomers-templates stands where on every input sequence, one row per block, to FILE (which must not exist yet)", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers},
    {"monomers-templates", 0, "FASTA", "With --monomers (required), the monomer templates: 1 to 1024 bases each, at most 8192 in all (both strands counted)", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_templates},
    {"monomers-summary", 0, "FILE", "With --monomers, write blocks, bases and score per sequence, template and strand to FILE (which must not exist yet)", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_summary},
    {"monomers-strands", 0, "WORD", "With --monomers, the strands of the templates that are tried: forward or both [forward]", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_strands},
    {"monomers-match", 0, "INT", "With --monomers, the score of a match, 1 to 64 [1]", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_match},
    {"monomers-mismatch", 0, "INT", "With --monomers, the score of a mismatch, -64 to -1 [-1]", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_mismatch},
    {"monomers-insertion", 0, "INT", "With --monomers, the score of a sequence base next to no template base, -64 to -1 [-1]", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_insertion},
    {"monomers-deletion", 0, "INT", "With --monomers, the score of a template base next to no sequence base, -64 to -1 [-1]", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_deletion},
    {"monomers-chunk", 0, "INT", "With --monomers, the bases of a sequence that are decomposed at once, 64 to 1048576, or 0 for all of them [4096]", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_chunk},
    {"monomers-overlap", 0, "INT", "With --monomers, the bases a chunk reads beyond either end, 0 to 1048576; two template lengths or more [512]", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_overlap},
    {"monomers-only", 0, NO, "With --monomers, end after writing the decomposition: nothing is aligned or printed", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_only},
    {"monomers-rounds", 0, "INT", "With --monomers, refine the templates in up to INT rounds (1 to 64) of decompose, align, vote before the decomposition is written", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_rounds},
    {"monomers-write-templates", 0, "FASTA", "With --monomers-rounds or seeds, write the final templates to FASTA (which must not exist yet)", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_write_templates},
    {"monomers-pileup", 0, "FILE", "With --monomers, write the per-column base counts of the blocks under the final templates to FILE (which must not exist yet)", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_pileup},
    {"monomers-least-share", 0, "INT", "With --monomers, the per mille of match * length a block's score must reach to be counted, 0 to 1000 [0]", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_least_share},
    {"monomers-seed-period", 0, "INT", "With --monomers, cut the templates from the first sequence, INT bases each (1 to 1024), instead of --monomers-templates", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_seed_period},
    {"monomers-seed-count", 0, "INT", "With --monomers-seed-period, the number of templates cut [1]", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_seed_count},
    {"monomers-seed-start", 0, "INT", "With --monomers-seed-period, the base of the first sequence at which the first template begins [0]", false, ADDED, GROUP_MONOMERS, NO, NO, &Options::monomers_seed_start},
    {"help", 'h', NO, "Print this message and exit", false, REF, GROUP_NONE, NO, NO, &Options::help},
};
const int ID_BASE = 1000;

void print_help(const cl_config* defaults) {
    FILE* o = stderr;
    fprintf(o, "\n");
    fprintf(o, "Usage: centrolign [options] sequences.fasta\n");
    fprintf(o, "\n");
    fprintf(o, "Aligns the sequences of a FASTA file (- reads standard input) on an AMD Instinct GPU and writes the alignment to standard\n");
    fprintf(o, "output: a CIGAR for two sequences, a GFA graph otherwise.\n");
    fprintf(o, "\n");
    fprintf(o, "Options:\n");
    std::vector<const Opt*> added;
    for (const Opt& row : TABLE) {
        std::string left = std::string(" --") + row.name + (row.letter ? std::string(" / -") + row.letter : "") + (row.meta ? std::string(" ") + row.meta : "");
        left.resize(std::max<size_t>(left.size() + 2, 29), ' ');
        fprintf(o, "%s%s%s\n", left.c_str(), row.help, row.shows_default ? (" [" + config_value(defaults, row.param) + "]").c_str() : "");
        if (!row.reference) added.push_back(&row);
    }
    fprintf(o, "\n");
    fprintf(o, "Differences from the reference centrolign: every failure is 'error: ...' with exit status 1; -p takes a decimal number;\n");
    std::string rest = "-t sets worker contexts;";   // ... and the added options, in lines of 133 characters at the most
    for (size_t i = 0; i < added.size(); ++i)
        rest += std::string(" --") + added[i]->name +
                (i + 2 < added.size() ? "," : i + 2 == added.size() ? " and" : " are added; -v gates this tool's own progress lines. See README.md.");
    size_t at = 0;
    for (; rest.size() - at > 133; at = rest.rfind(' ', at + 133) + 1) fprintf(o, "%s\n", rest.substr(at, rest.rfind(' ', at + 133) - at).c_str());
    fprintf(o, "%s\n", rest.c_str() + at);
}

// ---- what the outputs read ----------------------------------------------------------------------------------------------------------------

// a parsed FASTA with the names its sequences are shown under: as --pair-stats names them
struct Fasta {
    cl_fasta fa;
    bool parsed = false;
    std::vector<std::string> shown;
    std::vector<const char*> names;
    Fasta() = default;
    Fasta(const Fasta&) = delete;
    Fasta& operator=(const Fasta&) = delete;
    ~Fasta() { clear(); }
    bool parse(const std::string& text) {
        if (cl_parse_fasta(nullptr, text.data(), text.size(), &fa)) return false;
        parsed = true;
        for (uint64_t i = 0; i < fa.n_sequences; ++i) shown.push_back(flat_name(fa.names[i]));
        for (const std::string& nm : shown) names.push_back(nm.c_str());
        return true;
    }
    void clear() {
        if (parsed) cl_fasta_free(&fa);
        parsed = false;
    }
};

// a GFA text as the graph the outputs after the alignment read (cl_read_gfa, as cl_refine_guide_tree does) with its path names
struct NamedGraph {
    cl_owned_base_graph* owned = nullptr;
    cl_base_graph g;
    std::vector<std::string> names;
    NamedGraph() = default;
    NamedGraph(const NamedGraph&) = delete;
    NamedGraph& operator=(const NamedGraph&) = delete;
    ~NamedGraph() { if (owned) cl_owned_base_graph_free(owned); }
    bool load(const char* text, uint64_t len) {
        char** path_names = nullptr;
        uint64_t n_paths = 0;
        if (cl_read_gfa(text, len, 1, &owned, &path_names, &n_paths)) return false;
        for (uint64_t p = 0; p < n_paths; ++p) { names.emplace_back(path_names[p]); free(path_names[p]); }
        free(path_names);
        cl_owned_base_graph_view(owned, &g);
        return true;
    }
    uint64_t steps(uint64_t p) const { return g.path_off[p + 1] - g.path_off[p]; }
    const std::string* repeated_name() const {   // a name two paths carry: a sequence could not be found by it
        std::vector<const std::string*> sorted;
        for (const std::string& nm : names) sorted.push_back(&nm);
        std::sort(sorted.begin(), sorted.end(), [](const std::string* x, const std::string* y) { return *x < *y; });
        for (size_t i = 1; i < sorted.size(); ++i) if (*sorted[i] == *sorted[i - 1]) return sorted[i];
        return nullptr;
    }
    bool has_cycles() const {   // a path that meets a node twice
        std::vector<uint64_t> seen(g.n_nodes, 0);
        for (uint64_t p = 0; p < g.n_paths; ++p)
            for (uint64_t i = g.path_off[p]; i < g.path_off[p + 1]; ++i) {
                if (seen[g.path_nodes[i]] == p + 1) return true;
                seen[g.path_nodes[i]] = p + 1;
            }
        return false;
    }
};

// the monomer templates: of --monomers-templates, or cut by --monomers-seed-period
struct MonomerTemplates {
    std::vector<std::string> names, bases;
    std::vector<const char*> name_ptr, base_ptr;
    std::vector<uint64_t> lengths;
    void add(const char* name, const char* text, uint64_t len) {
        names.push_back(name);
        bases.push_back(std::string(text, len));
        lengths.push_back(len);
    }
    void point() {   // after the last change to names and bases
        name_ptr.clear();
        base_ptr.clear();
        for (size_t m = 0; m < names.size(); ++m) { name_ptr.push_back(names[m].c_str()); base_ptr.push_back(bases[m].c_str()); }
    }
};

// the templates of --monomers-templates, held to the library's limits (host only)
bool read_monomer_templates(const std::string& file, int strands, MonomerTemplates& t, std::string& err) {
    std::string text;
    {
        std::ifstream in(file, std::ios::binary);
        if (!in) { err = "--monomers-templates: cannot open " + file; return false; }
        text.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    }
    Fasta f;
    if (!f.parse(text)) { err = "--monomers-templates " + file + ": " + lib_error(); return false; }
    const cl_fasta& fa = f.fa;
    if (fa.n_sequences < 1) { err = "--monomers-templates " + file + " holds no template"; return false; }
    uint64_t total = 0;
    for (uint64_t m = 0; m < fa.n_sequences; ++m) {
        if (fa.lengths[m] < 1 || fa.lengths[m] > 1024) {
            err = "--monomers-templates: template " + std::string(fa.names[m]) + " has " + std::to_string(fa.lengths[m]) + " bases, not 1 to 1024";
            return false;
        }
        total += fa.lengths[m] * (uint64_t)strands;
        t.add(fa.names[m], fa.sequences[m], fa.lengths[m]);
    }
    if (total > 8192) { err = "--monomers-templates: " + std::to_string(total) + " template bases in all (both strands counted), more than 8192"; return false; }
    t.point();
    return true;
}

// ---- a run: what the stages hand on ---------------------------------------------------------------------------------------------------------

struct Run {
    int argc;
    char** argv;
    cl_config* cfg = cl_config_default();
    cl_config* defaults = cl_config_default();
    cl_context* ctx = nullptr;
    Options opt;
    std::vector<int> devices;
    int n_positional = 0;
    // the options as values
    cl_dotplot_params dotplot;
    cl_periods_params periods;
    int periods_scope = 0;
    cl_monomers_params monomers;
    MonomerTemplates templates;
    uint32_t monomer_rounds = 0, monomer_least_share = 0;
    uint64_t seed_period = 0, seed_count = 1, seed_start = 0;   // period 0: no seeds
    int refine_rounds = 0, msa_layout = 0;
    uint64_t window = 1000, min_event = 50, site_min_minor = 1, site_max_gaps = 0xFFFFFFFFull;
    NamedGraph baseline, given;
    std::string dist_tmp, stats_file;   // where --dist-out's rows pass through
    // the inputs
    std::string fasta_name, tree_name, fasta_text, newick;
    Fasta input;   // until the sequence outputs are written
    std::vector<std::string> sequence_names;
    uint64_t n_sequences = 0, n_bases = 0;
    bool have_tree = false;   // false: cl_msa gets NULL, the sequences in FASTA order
    cl_msa_params mp;
    cl_msa_stats st;

    Run(int argc_, char** argv_) : argc(argc_), argv(argv_) {
        cl_dotplot_params_default(&dotplot);
        cl_periods_params_default(&periods);
        cl_monomers_params_default(&monomers);
        memset(&st, 0, sizeof(st));
    }
    Run(const Run&) = delete;
    Run& operator=(const Run&) = delete;
    ~Run() {
        if (ctx) cl_context_destroy(ctx);
        cl_config_free(cfg);
        cl_config_free(defaults);
    }
    std::string config(const char* name) const { return config_value(cfg, name); }
    bool cyclizes() const { return config("cyclize_tandem_duplications") == "true"; }
    bool pair_positions() const { return !opt.pair_profile.empty() || !opt.pair_events.empty(); }
    bool agreement() const { return !opt.pair_agreement.empty(); }
    bool msa_columns() const { return !opt.msa_out.empty() || !opt.column_stats.empty() || !opt.variable_sites.empty(); }
    // the outputs of the alignment that the sequence outputs are compared with
    std::vector<std::string> alignment_outputs() const {
        return {opt.tree_out.text, opt.pair_stats.text, opt.dist_out.text, opt.pair_profile.text, opt.pair_events.text, opt.pair_agreement.text, opt.msa_out.text,
                opt.column_stats.text, opt.variable_sites.text, config("subalignments_filepath")};
    }
};

const int GO_ON = -1;   // what a stage returns that does not end the run; otherwise the exit status

int usage_error(const Run& r, const std::string& msg) {
    fprintf(stderr, "error: %s\n", msg.c_str());
    print_help(r.defaults);
    return 1;
}

int open_device(Run& r) {
    r.ctx = cl_context_create(r.devices.empty() ? 0 : r.devices[0]);
    return r.ctx ? GO_ON : fail("no usable GPU: " + lib_error());
}

// "--x expects <what>, got '<text>'"
std::string expects(const char* option, const std::string& what, const Given& g) { return std::string(option) + " expects " + what + ", got '" + g.text + "'"; }

// an option that is a whole number from least to most -> into; false if it was given and is none.  Not given: into stays
template <class T>
bool take_whole(const Given& g, long long least, long long most, T& into, bool as_strtol = false) {
    long long v = 0;
    if (!g.given) return true;
    if (!parse_whole(g.text, least, most, as_strtol, v)) return false;
    into = (T)v;
    return true;
}

// an option that is one of a few words -> the word's place among them; -1 if it is none of them
int word_of(const Given& g, std::initializer_list<const char*> words) {
    int at = 0;
    for (const char* w : words) {
        if (g.text == w) return at;
        ++at;
    }
    return -1;
}

// the first of these options that was given: the one a "needs --x" message names
const char* first_given(std::initializer_list<std::pair<const char*, bool>> options) {
    for (const auto& o : options) if (o.second) return o.first;
    return nullptr;
}

// ---- the outputs --------------------------------------------------------------------------------------------------------------------------

// --dist-out: the rows of a --pair-stats file (pairs (p, q), p < q, of the root graph's paths, named as -A names its files) -> cl_alignment_distances
// -> the matrix in FASTA order: a line with n, then per sequence its name and n values
bool write_distances(const std::string& stats_file, const std::vector<std::string>& names, const std::string& dist_file, std::string& err) {
    const uint64_t n = names.size();
    std::ifstream in(stats_file, std::ios::binary);
    std::string line;
    std::vector<cl_pair_stats> stats;
    std::vector<std::string> path_names;
    if (!in || !std::getline(in, line)) { err = "could not read the pair statistics from " + stats_file; return false; }
    while (std::getline(in, line)) {
        std::vector<std::string> f;
        for (size_t at = 0;;) {
            const size_t e = line.find('\t', at);
            f.push_back(line.substr(at, e == std::string::npos ? e : e - at));
            if (e == std::string::npos) break;
            at = e + 1;
        }
        if (f.size() != 11) { err = "unexpected line in " + stats_file + ": " + line; return false; }
        if (stats.empty()) path_names.push_back(f[0]);
        if (stats.size() + 1 < n) path_names.push_back(f[1]);
        cl_pair_stats s;
        uint64_t* v[8] = {&s.eq, &s.x, &s.ins, &s.del, &s.eq_runs, &s.x_runs, &s.ins_runs, &s.del_runs};
        for (int i = 0; i < 8; ++i) *v[i] = strtoull(f[2 + i].c_str(), nullptr, 10);
        stats.push_back(s);
    }
    if (stats.size() != n * (n - 1) / 2 || path_names.size() != n) { err = stats_file + " does not hold every pair of sequences"; return false; }
    std::vector<uint64_t> seq_of(n, n);   // path -> FASTA index, by the name -A gives the sequence
    for (uint64_t q = 0; q < n; ++q) {
        const std::string nm = flat_name(names[q]);
        uint64_t p = 0;
        while (p < n && path_names[p] != nm) ++p;
        if (p == n || seq_of[p] != n) { err = "sequence " + names[q] + " has no rows of its own in " + stats_file + " (names that differ only in '/' and '_' share one)"; return false; }
        seq_of[p] = q;
    }
    std::vector<double> by_path(n * n), by_seq(n * n);
    if (cl_alignment_distances(stats.data(), n, by_path.data())) { err = "could not compute the alignment distances"; return false; }
    for (uint64_t p = 0; p < n; ++p)
        for (uint64_t q = 0; q < n; ++q) by_seq[seq_of[p] * n + seq_of[q]] = by_path[p * n + q];
    std::string text = std::to_string(n) + "\n";
    for (uint64_t a = 0; a < n; ++a) {
        text += names[a];
        for (uint64_t b = 0; b < n; ++b) {
            char num[40];
            snprintf(num, sizeof(num), "\t%.9g", by_seq[a * n + b]);
            text += num;
        }
        text += '\n';
    }
    return write_file(dist_file, text, "the distance matrix", err);
}

// --pair-profile / --pair-events: every pair (p, q), p < q, of the printed graph's paths goes through the batch entry points; names as --pair-stats
// writes them
bool write_pair_positions(const Run& r, const NamedGraph& printed, std::string& err) {
    const cl_base_graph& g = printed.g;
    const uint64_t n_paths = printed.names.size();
    std::vector<std::string> names;
    for (const std::string& nm : printed.names) names.push_back(flat_name(nm));
    std::vector<uint64_t> pairs;
    for (uint64_t p = 0; p < n_paths; ++p)
        for (uint64_t q = p + 1; q < n_paths; ++q) { pairs.push_back(p); pairs.push_back(q); }
    const uint64_t n_pairs = pairs.size() / 2;
    std::vector<uint64_t> off(n_pairs + 1);
    if (!r.opt.pair_profile.empty()) {
        cl_pair_window* win = nullptr;
        if (cl_induced_pairwise_profiles(r.ctx, &g, pairs.data(), n_pairs, r.window, &win, off.data())) {
            err = context_error(r.ctx, "pairwise profiles of the alignment graph");
            return false;
        }
        std::string tsv = "sample1\tsample2\twindow_start\twindow_end\tmatches\tmismatches\tinsertions\tdeletions\n";
        for (uint64_t k = 0; k < n_pairs; ++k) {
            const uint64_t n1 = printed.steps(pairs[2 * k]);
            const std::string lead = names[pairs[2 * k]] + "\t" + names[pairs[2 * k + 1]];
            for (uint64_t w = 0; w < off[k + 1] - off[k]; ++w) {
                const cl_pair_window& c = win[off[k] + w];
                char num[160];
                snprintf(num, sizeof(num), "\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)std::min(w * r.window, n1),
                         (unsigned long long)std::min((w + 1) * r.window, n1), (unsigned long long)c.eq, (unsigned long long)c.x, (unsigned long long)c.ins,
                         (unsigned long long)c.del);
                tsv += lead;
                tsv += num;
            }
        }
        free(win);
        if (!write_file(r.opt.pair_profile.text, tsv, "", err)) return false;
    }
    if (!r.opt.pair_events.empty()) {
        cl_gap_event* ev = nullptr;
        if (cl_induced_gap_events_batch(r.ctx, &g, pairs.data(), n_pairs, r.min_event, &ev, off.data())) {
            err = context_error(r.ctx, "gap events of the alignment graph");
            return false;
        }
        std::string tsv = "sample1\tsample2\ttype\tpos1\tpos2\tlength\n";
        for (uint64_t k = 0; k < n_pairs; ++k) {
            const std::string lead = names[pairs[2 * k]] + "\t" + names[pairs[2 * k + 1]];
            for (uint64_t i = off[k]; i < off[k + 1]; ++i) {
                char num[128];
                snprintf(num, sizeof(num), "\t%c\t%llu\t%llu\t%llu\n", ev[i].op ? 'I' : 'D', (unsigned long long)ev[i].pos1, (unsigned long long)ev[i].pos2,
                         (unsigned long long)ev[i].len);
                tsv += lead;
                tsv += num;
            }
        }
        free(ev);
        if (!write_file(r.opt.pair_events.text, tsv, "", err)) return false;
    }
    return true;
}

// --msa-out / --column-stats / --variable-sites: the printed graph goes through one cl_msa_columns_compute call that makes what the files named
// need; entries in the printed graph's path order under the paths' names
bool write_msa_columns(const Run& r, const NamedGraph& printed, std::string& err) {
    const std::string &msa_file = r.opt.msa_out.text, &stats_file = r.opt.column_stats.text, &sites_file = r.opt.variable_sites.text;
    cl_msa_columns_params params;
    cl_msa_columns_params_default(&params);
    params.layout = r.msa_layout;
    params.want = (msa_file.empty() ? 0u : 1u) | (stats_file.empty() ? 0u : 2u) | (sites_file.empty() ? 0u : 4u);
    params.min_minor = (uint32_t)r.site_min_minor;
    params.max_gaps = (uint32_t)r.site_max_gaps;
    const auto t0 = std::chrono::steady_clock::now();
    cl_msa_columns m;
    if (cl_msa_columns_compute(r.ctx, &printed.g, &params, &m)) { err = context_error(r.ctx, "the alignment graph as columns"); return false; }
    struct FreeColumns { cl_msa_columns* m; ~FreeColumns() { cl_msa_columns_free(m); } } free_columns{&m};
    char line[200];
    snprintf(line, sizeof(line), "The alignment as columns (%s layout): %llu column(s)%s in %.3f s.", r.msa_layout == 0 ? "level" : "node", (unsigned long long)m.n_cols,
             sites_file.empty() ? "" : (", " + std::to_string(m.n_sites) + " variable site(s)").c_str(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    log_line(LOG_VERBOSE, line);
    auto fasta = [&](const char* rows, uint64_t width) {
        std::string text;
        for (uint64_t p = 0; p < printed.names.size(); ++p) {
            text += '>'; text += printed.names[p]; text += '\n';
            text.append(rows + p * width, width);
            text += '\n';
        }
        return text;
    };
    if (!msa_file.empty() && !write_file(msa_file, fasta(m.rows, m.n_cols), "", err)) return false;
    if (!stats_file.empty()) {
        std::string tsv = "column\tA\tC\tG\tT\tN\tgaps\tconsensus\tsite\n";
        for (uint64_t c = 0; c < m.n_cols; ++c) {
            const cl_msa_column& col = m.columns[c];
            char num[160];
            snprintf(num, sizeof(num), "%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%c\t%u\n", (unsigned long long)c, col.count[0], col.count[1], col.count[2], col.count[3], col.count[4],
                     col.gaps, "ACGTN-"[col.consensus], col.flags & 1u);
            tsv += num;
        }
        if (!write_file(stats_file, tsv, "", err)) return false;
    }
    return sites_file.empty() || write_file(sites_file, fasta(m.site_rows, m.n_sites), "", err);
}

// --compare-to / --pair-agreement: every pair (p, q), p < q, of the printed graph's paths against the same two sequences in the baseline, found there
// by name; names as --pair-stats writes them.  The baseline is graph a of cl_induced_pairwise_agreements: aligned_base, matches_base are its columns
bool write_pair_agreement(const Run& r, const NamedGraph& printed, std::string& err) {
    const NamedGraph& base = r.baseline;
    const uint64_t n = printed.names.size();
    std::vector<uint64_t> in_base(n);
    for (uint64_t p = 0; p < n; ++p) {
        const auto it = std::find(base.names.begin(), base.names.end(), printed.names[p]);
        if (it == base.names.end()) { err = "the baseline graph has no path " + printed.names[p]; return false; }
        const uint64_t q = (uint64_t)(it - base.names.begin());
        bool same = printed.steps(p) == base.steps(q);
        for (uint64_t i = 0; same && i < printed.steps(p); ++i)
            same = printed.g.label[printed.g.path_nodes[printed.g.path_off[p] + i]] == base.g.label[base.g.path_nodes[base.g.path_off[q] + i]];
        if (!same) { err = "path " + printed.names[p] + " spells another sequence in the baseline graph"; return false; }
        in_base[p] = q;
    }
    std::vector<uint64_t> quads;
    for (uint64_t p = 0; p < n; ++p)
        for (uint64_t q = p + 1; q < n; ++q) quads.insert(quads.end(), {in_base[p], in_base[q], p, q});
    const uint64_t n_quads = quads.size() / 4;
    std::vector<cl_pair_agreement> got(n_quads);
    if (cl_induced_pairwise_agreements(r.ctx, &base.g, &printed.g, quads.data(), n_quads, got.data())) {
        err = context_error(r.ctx, "agreement with the baseline graph");
        return false;
    }
    std::string tsv = "sample1\tsample2\taligned_base\taligned\tshared\tmatches_base\tmatches\tshared_matches\n";
    uint64_t aligned_base = 0, aligned = 0, shared = 0;
    for (uint64_t k = 0; k < n_quads; ++k) {
        const cl_pair_agreement& a = got[k];
        char num[200];
        snprintf(num, sizeof(num), "\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)a.aligned_a, (unsigned long long)a.aligned_b,
                 (unsigned long long)a.shared, (unsigned long long)a.eq_a, (unsigned long long)a.eq_b, (unsigned long long)a.shared_eq);
        tsv += flat_name(printed.names[quads[4 * k + 2]] + "\t" + printed.names[quads[4 * k + 3]]);
        tsv += num;
        aligned_base += a.aligned_a; aligned += a.aligned_b; shared += a.shared;
    }
    if (!write_file(r.opt.pair_agreement.text, tsv, "", err)) return false;
    char line[256];
    snprintf(line, sizeof(line), "Agreement with the baseline over %llu pair(s): recall %.6f (%llu shared of %llu aligned there), precision %.6f (of %llu aligned here).",
             (unsigned long long)n_quads, aligned_base ? (double)shared / (double)aligned_base : 1.0, (unsigned long long)shared, (unsigned long long)aligned_base,
             aligned ? (double)shared / (double)aligned : 1.0, (unsigned long long)aligned);
    log_line(LOG_BASIC, line);
    return true;
}

// --dotplot: the windowed k-mer identity map of the input's sequences
bool write_dotplot(Run& r, std::string& err) {
    const cl_fasta& fa = r.input.fa;
    cl_dotplot plot;
    if (cl_kmer_dotplot_compute(r.ctx, fa.sequences, fa.lengths, fa.n_sequences, &r.dotplot, &plot)) { err = context_error(r.ctx, "the dot plot"); return false; }
    struct FreePlot { cl_dotplot* d; ~FreePlot() { cl_dotplot_free(d); } } free_plot{&plot};
    char line[256];
    snprintf(line, sizeof(line), "The dot plot: %llu windows of %u bases, %llu entries; k-mer lists %.3f ms, window pairs %.3f ms on the device.",
             (unsigned long long)plot.n_windows, plot.window, (unsigned long long)plot.n_entries, plot.spectra_ms, plot.pairs_ms);
    log_line(LOG_VERBOSE, line);
    LibText t;
    if (cl_dotplot_tsv(&plot, r.input.names.data(), fa.lengths, &t.text, &t.len)) { err = "the dot plot: " + lib_error(); return false; }
    return write_file(r.opt.dotplot.text, t.text, t.len, "the dot plot", err);
}

// --periods / --periods-hist: the repeat period spectra of the input's sequences
bool write_periods(Run& r, std::string& err) {
    const cl_fasta& fa = r.input.fa;
    cl_period_spectrum spec;
    if (cl_period_spectrum_compute(r.ctx, fa.sequences, fa.lengths, fa.n_sequences, &r.periods, &spec)) { err = context_error(r.ctx, "the period spectra"); return false; }
    struct FreeSpectrum { cl_period_spectrum* d; ~FreeSpectrum() { cl_period_spectrum_free(d); } } free_spectrum{&spec};
    uint64_t n_links = 0;
    for (uint64_t s = 0; s < spec.n_seq; ++s) n_links += spec.links[spec.n_windows + s];
    char line[256];
    snprintf(line, sizeof(line), "The period spectra: %llu rows of %u bins, %llu links; links %.3f ms, histograms %.3f ms on the device.",
             (unsigned long long)spec.n_rows, spec.max_period + 1, (unsigned long long)n_links, spec.links_ms, spec.hist_ms);
    log_line(LOG_VERBOSE, line);
    for (const Given* to : {&r.opt.periods, &r.opt.periods_hist}) {
        if (to->empty()) continue;
        LibText t;
        if ((to == &r.opt.periods ? cl_periods_tsv : cl_periods_hist_tsv)(&spec, r.input.names.data(), fa.lengths, r.periods_scope, &t.text, &t.len)) {
            err = "the period spectra: " + lib_error();
            return false;
        }
        if (!write_file(to->text, t.text, t.len, "the period spectra", err)) return false;
    }
    return true;
}

// --monomers / --monomers-summary and what goes with them: the monomer decomposition of the input's sequences
bool write_monomers(Run& r, std::string& err) {
    const cl_fasta& fa = r.input.fa;
    const cl_monomers_params& params = r.monomers;
    MonomerTemplates t = r.templates;   // the final templates: the given ones unless rounds are asked for
    char line[320];
    if (r.monomer_rounds) {
        cl_monomer_templates refined;
        if (cl_monomer_templates_refine_compute(r.ctx, fa.sequences, fa.lengths, fa.n_sequences, r.templates.base_ptr.data(), r.templates.lengths.data(), r.templates.lengths.size(),
                                                &params, r.monomer_least_share, r.monomer_rounds, &refined)) {
            err = context_error(r.ctx, "the template refinement");
            return false;
        }
        for (uint32_t i = 0; i < refined.rounds; ++i) {
            const cl_monomer_round& q = refined.round[i];
            snprintf(line, sizeof(line), "Template round %u: %llu blocks, %llu used, %llu templates changed; rows %.3f ms, blocks %.3f ms, alignments %.3f ms, counts %.3f ms on the device.",
                     i + 1, (unsigned long long)q.blocks, (unsigned long long)q.used, (unsigned long long)q.changed, q.dp_ms, q.trace_ms, q.align_ms, q.count_ms);
            log_line(LOG_VERBOSE, line);
        }
        snprintf(line, sizeof(line), "The templates %s after %u round(s).", refined.converged ? "converged" : "did not converge", refined.rounds);
        log_line(LOG_VERBOSE, line);
        for (size_t m = 0; m < t.bases.size(); ++m) { t.bases[m].assign(refined.templates[m], refined.lengths[m]); t.lengths[m] = refined.lengths[m]; }
        cl_monomer_templates_free(&refined);
    }
    t.point();
    if (!r.opt.monomers_write_templates.empty()) {
        LibText text;
        if (cl_monomer_templates_fasta(t.name_ptr.data(), t.base_ptr.data(), t.lengths.data(), t.lengths.size(), &text.text, &text.len)) { err = "the templates: " + lib_error(); return false; }
        if (!write_file(r.opt.monomers_write_templates.text, text.text, text.len, "the templates", err)) return false;
    }
    cl_monomer_decomposition dec;
    if (cl_monomer_decompose_compute(r.ctx, fa.sequences, fa.lengths, fa.n_sequences, t.base_ptr.data(), t.lengths.data(), t.lengths.size(), &params, &dec)) {
        err = context_error(r.ctx, "the monomer decomposition");
        return false;
    }
    struct FreeDecomposition { cl_monomer_decomposition* d; ~FreeDecomposition() { cl_monomer_decomposition_free(d); } } free_decomposition{&dec};
    snprintf(line, sizeof(line), "The monomer decomposition: %llu problems, %llu blocks; rows %.3f ms, blocks %.3f ms on the device.",
             (unsigned long long)dec.n_problems, (unsigned long long)dec.n_blocks, dec.dp_ms, dec.trace_ms);
    log_line(LOG_VERBOSE, line);
    if (!r.opt.monomers_pileup.empty()) {
        cl_monomer_pileup pile;
        if (cl_monomer_pileup_compute(r.ctx, fa.sequences, fa.lengths, fa.n_sequences, t.base_ptr.data(), t.lengths.data(), t.lengths.size(), &params, &dec,
                                      r.monomer_least_share, &pile)) {
            err = context_error(r.ctx, "the monomer pileup");
            return false;
        }
        uint64_t used = 0;
        for (uint64_t m = 0; m < pile.n_templates; ++m) used += pile.used[m];
        snprintf(line, sizeof(line), "The monomer pileup: %llu blocks used; alignments %.3f ms, counts %.3f ms on the device.", (unsigned long long)used, pile.align_ms,
                 pile.count_ms);
        log_line(LOG_VERBOSE, line);
        LibText text;
        const int rc = cl_monomer_pileup_tsv(&pile, t.name_ptr.data(), t.base_ptr.data(), t.lengths.data(), t.lengths.size(), &text.text, &text.len);
        cl_monomer_pileup_free(&pile);
        if (rc) { err = "the monomer pileup: " + lib_error(); return false; }
        if (!write_file(r.opt.monomers_pileup.text, text.text, text.len, "the monomer pileup", err)) return false;
    }
    for (const Given* to : {&r.opt.monomers, &r.opt.monomers_summary}) {
        if (to->empty()) continue;
        LibText text;
        if ((to == &r.opt.monomers ? cl_monomers_tsv : cl_monomers_summary_tsv)(&dec, r.input.names.data(), t.name_ptr.data(), t.lengths.data(), t.lengths.size(), &params,
                                                                                 &text.text, &text.len)) {
            err = "the monomer decomposition: " + lib_error();
            return false;
        }
        if (!write_file(to->text, text.text, text.len, "the monomer decomposition", err)) return false;
    }
    return true;
}

// the outputs that read the input sequences alone, in the order they are written in
const struct SequenceOutput {
    const char* option;   // --x; --x-only ends the run after it
    Group group;
    Given Options::* file;
    Given Options::* only;
    const char* what;
    bool (*write)(Run&, std::string&);
} SEQUENCE_OUTPUTS[3] = {
    {"--dotplot", GROUP_DOTPLOT, &Options::dotplot, &Options::dotplot_only, "the dot plot", write_dotplot},
    {"--periods", GROUP_PERIODS, &Options::periods, &Options::periods_only, "the period spectra", write_periods},
    {"--monomers", GROUP_MONOMERS, &Options::monomers, &Options::monomers_only, "the monomer decomposition", write_monomers},
};

// ---- the stages, in the order run() goes through them ----------------------------------------------------------------------------------------

// the command line -> the config and the options.  What is wrong with an option is reported where the option stands, and -h acts there
int parse_command_line(Run& r) {
    std::vector<option> longs;
    std::string shorts = ":";
    for (const Opt& row : TABLE) {
        longs.push_back({row.name, row.meta ? required_argument : no_argument, nullptr, ID_BASE + (int)(&row - TABLE)});
        if (row.letter) shorts += std::string(1, row.letter) + (row.meta ? ":" : "");
    }
    longs.push_back({nullptr, 0, nullptr, 0});
    opterr = 0;   // reported here, as "error: ..."
    while (true) {
        const int o = getopt_long(r.argc, r.argv, shorts.c_str(), longs.data(), nullptr);
        if (o == -1) break;
        const Opt* row = o >= ID_BASE ? &TABLE[o - ID_BASE] : nullptr;
        for (const Opt& t : TABLE) if (t.letter == o) row = &t;
        if (!row) {
            // optopt names a short option; a long one is the argument getopt just stepped over
            const std::string opt = optopt > 0 && optopt < 128 ? std::string("-") + (char)optopt : std::string(optind > 0 && optind <= r.argc ? r.argv[optind - 1] : "");
            return usage_error(r, o == ':' ? "option '" + opt + "' requires an argument" : "unknown option '" + opt + "'");
        }
        if (row->into == &Options::help) {
            print_help(r.defaults);
            return 0;
        }
        for (int g = GROUP_NONE + 1; g < N_GROUPS; ++g)
            if (row->letter != 'v' && row->into != &Options::devices && row->group != g) r.opt.beside_only[g] = true;
        if (row->into) {
            Given& g = r.opt.*row->into;
            g.given = true;
            if (optarg) g.text = optarg;
        }
        if (row->into == &Options::devices && !parse_devices(optarg, r.devices)) return fail(std::string("--devices expects comma-separated device ordinals, got '") + optarg + "'");
        if (row->param && cl_config_set(r.cfg, row->param, row->fixed ? row->fixed : optarg)) return fail(lib_error());
    }
    return GO_ON;
}

int take_positional(Run& r) {
    r.n_positional = r.argc - optind;
    if (r.n_positional > 1) return usage_error(r, "expected between 0 and 1 positional arguments but got " + std::to_string(r.n_positional));
    if (r.n_positional == 1 && cl_config_set(r.cfg, "fasta_name", r.argv[optind])) return fail(lib_error());
    return GO_ON;
}

int generate_config(Run& r) {
    if (!r.opt.generate_config.given) return GO_ON;
    const std::string text = generate(r.cfg);
    fwrite(text.data(), 1, text.size(), stdout);
    return fflush(stdout) == 0 ? 0 : fail("could not write the config to standard output");
}

// --graph stands in for the whole run: it goes with the two comparison options and with nothing that reads an input or writes another output
int check_graph_alone(Run& r) {
    const Options& o = r.opt;
    if (!o.graph.given) return GO_ON;
    if (o.compare_to.empty() || o.pair_agreement.empty()) return fail("--graph needs --compare-to and --pair-agreement");
    if (r.n_positional == 1) return fail("--graph cannot be combined with a FASTA: it takes the place of the alignment");
    if (!r.config("tree_name").empty() || o.infer_tree.given || !o.refine_tree.empty()) return fail("--graph cannot be combined with a guide tree (-T, --infer-tree, --refine-tree)");
    if (!o.config.empty()) return fail("--graph cannot be combined with a config file (-C)");
    if (r.config("restart") == "true") return fail("--graph cannot be combined with a restart (-R)");
    for (const char* name : {"all_pairs_prefix", "subproblems_prefix", "subalignments_filepath", "bonds_prefix"})
        if (!r.config(name).empty()) return fail("--graph cannot be combined with another output option (-A, -S, -s, --bond-prefix)");
    if (!o.tree_out.empty() || !o.pair_stats.empty() || !o.dist_out.empty() || r.pair_positions() || o.window.given || o.min_event.given)
        return fail("--graph cannot be combined with another output option (--tree-out, --pair-stats, --dist-out, --pair-profile, --pair-events)");
    if (r.msa_columns() || o.msa_layout.given || o.site_min_minor.given || o.site_max_gaps.given)
        return fail("--graph cannot be combined with another output option (--msa-out, --column-stats, --variable-sites)");
    return GO_ON;
}

int check_only_rule(Run& r) {
    for (const SequenceOutput& out : SEQUENCE_OUTPUTS)
        if ((r.opt.*out.only).given && !(r.opt.*out.file).empty() && r.opt.beside_only[out.group])
            return fail(std::string(out.option) + "-only goes with the " + out.option + " options, -v and --devices alone: nothing else is run");
    return GO_ON;
}

int load_config_file(Run& r) {
    if (r.opt.config.empty()) return GO_ON;
    if (generate(r.cfg) != generate(r.defaults))
        fprintf(stderr, "warning: All other command-line arguments are being overridden by config file parameters.\n\n");
    std::string text, err;
    if (!read_input(r.opt.config.text, text, err)) return fail(err);
    cl_config* parsed = nullptr;
    if (cl_config_parse(text.data(), text.size(), &parsed)) return fail(lib_error());
    cl_config_free(r.cfg);
    r.cfg = parsed;
    return GO_ON;
}

// --dotplot and its options, checked before anything is read or opened
int check_dotplot(Run& r) {
    const Options& o = r.opt;
    cl_dotplot_params& p = r.dotplot;
    std::string err;
    if (o.dotplot.empty()) {
        const char* lone = first_given({{"--dotplot-k", o.dotplot_k.given}, {"--dotplot-window", o.dotplot_window.given}, {"--dotplot-min-identity", o.dotplot_min_identity.given},
                                        {"--dotplot-pairs", o.dotplot_pairs.given}, {"--dotplot-only", o.dotplot_only.given}});
        return lone ? fail(std::string(lone) + " needs --dotplot") : GO_ON;
    }
    if (o.graph.given) return fail("--dotplot cannot be combined with --graph: it reads the sequences of a FASTA");
    if (!take_whole(o.dotplot_k, 1, 31, p.k)) return fail(expects("--dotplot-k", "a k-mer length from 1 to 31", o.dotplot_k));
    if (!take_whole(o.dotplot_window, std::max(p.k, 1), 1 << 20, p.window))
        return fail(expects("--dotplot-window", "a whole number of bases from k = " + std::to_string(p.k) + " to 1048576", o.dotplot_window));
    if (p.window < (uint32_t)p.k) return fail("--dotplot-k " + o.dotplot_k.text + " is more than the window of " + std::to_string(p.window) + " bases");
    if (o.dotplot_min_identity.given) {
        const std::string& text = o.dotplot_min_identity.text;
        char* end = nullptr;
        errno = 0;
        const double x = strtod(text.c_str(), &end);
        if (text.empty() || *end || errno || !(x >= 0.0 && x <= 100.0)) return fail(expects("--dotplot-min-identity", "a percentage from 0 to 100", o.dotplot_min_identity));
        p.min_identity = x;
    }
    if (o.dotplot_pairs.given && (p.pairs = word_of(o.dotplot_pairs, {"all", "self"})) < 0) return fail(expects("--dotplot-pairs", "all or self", o.dotplot_pairs));
    if (already_exists("Dot plot", o.dotplot.text, err)) return fail(err);
    if (clashes({o.dotplot.text}, r.alignment_outputs(), "--dotplot names the file of another output option", err)) return fail(err);
    return GO_ON;
}

// --periods and its options, checked the same way
int check_periods(Run& r) {
    const Options& o = r.opt;
    cl_periods_params& p = r.periods;
    const struct { const char* option; const Given& as_given; const char* what; long long most; uint32_t* into; } numbers[7] = {
        {"--periods-k", o.periods_k, "a k-mer length from 1 to 31", 31, nullptr},
        {"--periods-window", o.periods_window, "a whole number of bases from 1 to 1048576", 1 << 20, &p.window},
        {"--periods-max", o.periods_max, "a period from 1 to 16383", 16383, &p.max_period},
        {"--periods-peaks", o.periods_peaks, "a number of peaks from 1 to 16", 16, &p.n_peaks},
        {"--periods-radius", o.periods_radius, "a number of bins from 1 to 64", 64, &p.peak_radius},
        {"--periods-min-period", o.periods_min_period, "a period, at least 1", 0xFFFFFFFFll, &p.min_period},
        {"--periods-min-count", o.periods_min_count, "a count, at least 1", 0xFFFFFFFFll, &p.min_count}};
    std::string err;
    if (o.periods.empty()) {
        const char* lone = first_given({{"--periods-hist", !o.periods_hist.empty()}, {"--periods-scope", o.periods_scope.given}, {"--periods-only", o.periods_only.given}});
        for (int i = 6; i >= 0; --i) if (numbers[i].as_given.given) lone = numbers[i].option;
        return lone ? fail(std::string(lone) + " needs --periods") : GO_ON;
    }
    if (o.graph.given) return fail("--periods cannot be combined with --graph: it reads the sequences of a FASTA");
    for (const auto& n : numbers)
        if (!(n.into ? take_whole(n.as_given, 1, n.most, *n.into) : take_whole(n.as_given, 1, n.most, p.k))) return fail(expects(n.option, n.what, n.as_given));
    if (o.periods_scope.given && (r.periods_scope = word_of(o.periods_scope, {"both", "sequences", "windows"})) < 0)
        return fail(expects("--periods-scope", "both, sequences or windows", o.periods_scope));
    p.want_hist = o.periods_hist.empty() ? 0 : 1;
    if (already_exists("Period spectra", o.periods.text, err) || already_exists("Period histogram", o.periods_hist.text, err)) return fail(err);
    if (o.periods.text == o.periods_hist.text) return fail("--periods and --periods-hist name the same file");
    std::vector<std::string> others = r.alignment_outputs();
    others.push_back(o.dotplot.text);
    if (clashes({o.periods.text, o.periods_hist.text}, others, "--periods and --periods-hist cannot name the file of another output option", err)) return fail(err);
    return GO_ON;
}

// --monomers and its options, checked the same way; the templates are read here: what is wrong with them needs no other input
int check_monomers(Run& r) {
    const Options& o = r.opt;
    cl_monomers_params& p = r.monomers;
    std::string err;
    if (o.monomers.empty()) {
        const char* lone = first_given({{"--monomers-rounds", o.monomers_rounds.given}, {"--monomers-write-templates", o.monomers_write_templates.given},
                                        {"--monomers-pileup", o.monomers_pileup.given}, {"--monomers-least-share", o.monomers_least_share.given},
                                        {"--monomers-seed-period", o.monomers_seed_period.given}, {"--monomers-seed-count", o.monomers_seed_count.given},
                                        {"--monomers-seed-start", o.monomers_seed_start.given}, {"--monomers-match", o.monomers_match.given},
                                        {"--monomers-mismatch", o.monomers_mismatch.given}, {"--monomers-insertion", o.monomers_insertion.given},
                                        {"--monomers-deletion", o.monomers_deletion.given}, {"--monomers-chunk", o.monomers_chunk.given},
                                        {"--monomers-overlap", o.monomers_overlap.given}, {"--monomers-templates", !o.monomers_templates.empty()},
                                        {"--monomers-summary", !o.monomers_summary.empty()}, {"--monomers-strands", o.monomers_strands.given},
                                        {"--monomers-only", o.monomers_only.given}});
        return lone ? fail(std::string(lone) + " needs --monomers") : GO_ON;
    }
    const bool seeds = o.monomers_seed_period.given;
    if (o.graph.given) return fail("--monomers cannot be combined with --graph: it reads the sequences of a FASTA");
    if (o.monomers_templates.empty() && !seeds) return fail("--monomers needs --monomers-templates or --monomers-seed-period");
    if (!o.monomers_templates.empty() && seeds) return fail("--monomers-templates and --monomers-seed-period cannot both be given");
    if (!seeds && (o.monomers_seed_count.given || o.monomers_seed_start.given))
        return fail(std::string(o.monomers_seed_count.given ? "--monomers-seed-count" : "--monomers-seed-start") + " needs --monomers-seed-period");
    if (o.monomers_write_templates.given && !o.monomers_rounds.given && !seeds)
        return fail("--monomers-write-templates needs --monomers-rounds or --monomers-seed-period: the given templates would be written back");
    if (!take_whole(o.monomers_match, 1, 64, p.match)) return fail(expects("--monomers-match", "a score from 1 to 64", o.monomers_match));
    const struct { const char* option; const Given& as_given; int32_t& into; } penalties[3] = {
        {"--monomers-mismatch", o.monomers_mismatch, p.mismatch}, {"--monomers-insertion", o.monomers_insertion, p.insertion}, {"--monomers-deletion", o.monomers_deletion, p.deletion}};
    for (const auto& n : penalties)
        if (!take_whole(n.as_given, -64, -1, n.into, true)) return fail(expects(n.option, "a score from -64 to -1", n.as_given));
    if (!take_whole(o.monomers_chunk, 0, 1 << 20, p.chunk) || (o.monomers_chunk.given && p.chunk != 0 && p.chunk < 64))
        return fail(expects("--monomers-chunk", "0 or a whole number of bases from 64 to 1048576", o.monomers_chunk));
    if (!take_whole(o.monomers_overlap, 0, 1 << 20, p.overlap)) return fail(expects("--monomers-overlap", "a whole number of bases from 0 to 1048576", o.monomers_overlap));
    if (o.monomers_strands.given && (p.strands = word_of(o.monomers_strands, {"forward", "both"}) + 1) < 1)
        return fail(expects("--monomers-strands", "forward or both", o.monomers_strands));
    if (already_exists("Monomer decomposition", o.monomers.text, err) || already_exists("Monomer summary", o.monomers_summary.text, err)) return fail(err);
    if (o.monomers.text == o.monomers_summary.text) return fail("--monomers and --monomers-summary name the same file");
    std::vector<std::string> others = r.alignment_outputs();
    others.insert(others.end(), {o.dotplot.text, o.periods.text, o.periods_hist.text});
    if (clashes({o.monomers.text, o.monomers_summary.text}, others, "--monomers and --monomers-summary cannot name the file of another output option", err) ||
        clashes({o.monomers.text, o.monomers_summary.text}, {o.monomers_templates.text}, "--monomers and --monomers-summary cannot name the templates' file", err))
        return fail(err);
    if (!take_whole(o.monomers_rounds, 1, 64, r.monomer_rounds)) return fail(expects("--monomers-rounds", "a whole number of rounds from 1 to 64", o.monomers_rounds));
    if (!take_whole(o.monomers_least_share, 0, 1000, r.monomer_least_share))
        return fail(expects("--monomers-least-share", "a whole number of per mille from 0 to 1000", o.monomers_least_share));
    if (seeds) {
        if (!take_whole(o.monomers_seed_period, 1, 1024, r.seed_period)) return fail(expects("--monomers-seed-period", "a whole number of bases from 1 to 1024", o.monomers_seed_period));
        if (!take_whole(o.monomers_seed_count, 1, 8192, r.seed_count)) return fail(expects("--monomers-seed-count", "a whole number of templates from 1 on", o.monomers_seed_count));
        if (r.seed_period * r.seed_count * (uint64_t)p.strands > 8192)
            return fail("--monomers-seed-count: " + std::to_string(r.seed_count) + " templates of " + std::to_string(r.seed_period) +
                        " bases are more than 8192 template bases in all (both strands counted)");
        if (!take_whole(o.monomers_seed_start, 0, (1ll << 30) - 1, r.seed_start)) return fail(expects("--monomers-seed-start", "a whole number of bases below 2^30", o.monomers_seed_start));
    }
    const struct { const char* option; const Given& made; const char* label; std::vector<std::string> siblings; } made_files[2] = {
        {"--monomers-write-templates", o.monomers_write_templates, "Monomer templates", {o.monomers.text, o.monomers_summary.text, o.monomers_templates.text}},
        {"--monomers-pileup", o.monomers_pileup, "Monomer pileup", {o.monomers.text, o.monomers_summary.text, o.monomers_templates.text, o.monomers_write_templates.text}}};
    for (const auto& m : made_files) {
        if (!m.made.given) continue;
        if (m.made.empty()) return fail(std::string(m.option) + " expects a file name");
        if (already_exists(m.label, m.made.text, err)) return fail(err);
        if (clashes({m.made.text}, m.siblings, std::string(m.option) + " cannot name the file of another --monomers option", err) ||
            clashes({m.made.text}, others, std::string(m.option) + " cannot name the file of another output option", err))
            return fail(err);
    }
    if (!o.monomers_templates.empty() && !read_monomer_templates(o.monomers_templates.text, p.strands, r.templates, err)) return fail(err);
    return GO_ON;
}

// the tree options of this project
int check_tree_options(Run& r) {
    const Options& o = r.opt;
    if (o.infer_tree.given && !r.config("tree_name").empty()) return fail("--infer-tree cannot be combined with a guide tree (-T or tree_name)");
    if (!o.tree_out.empty() && !o.infer_tree.given && o.refine_tree.empty()) return fail("--tree-out needs --infer-tree");
    if (!o.refine_tree.empty()) {
        long long v = 0;
        if (!parse_whole(o.refine_tree.text, 1, 1000000, true, v)) return fail(expects("--refine-tree", "a whole number of rounds, at least 1", o.refine_tree));
        r.refine_rounds = (int)v;
        if (r.config("restart") == "true") return fail("--refine-tree cannot be combined with a restart (-R)");
    }
    return GO_ON;
}

// --pair-stats, --pair-profile / --pair-events
int check_pair_outputs(Run& r) {
    const Options& o = r.opt;
    std::string err;
    if (already_exists("Pair statistics", o.pair_stats.text, err)) return fail(err);
    if (o.window.given && o.pair_profile.empty()) return fail("--window needs --pair-profile");
    if (o.min_event.given && o.pair_events.empty()) return fail("--min-event needs --pair-events");
    if (!take_whole(o.window, 1, LLONG_MAX, r.window)) return fail(expects("--window", "a whole number of bases, at least 1", o.window));
    if (!take_whole(o.min_event, 1, LLONG_MAX, r.min_event)) return fail(expects("--min-event", "a whole number of bases, at least 1", o.min_event));
    if (already_exists("Pair profile", o.pair_profile.text, err) || already_exists("Pair events", o.pair_events.text, err)) return fail(err);
    if (!o.pair_profile.empty() && o.pair_profile.text == o.pair_events.text) return fail("--pair-profile and --pair-events name the same file");
    if (r.pair_positions() && r.cyclizes()) return fail("--pair-profile and --pair-events cannot be combined with -c: the final graph then has cycles");
    return GO_ON;
}

// --compare-to / --pair-agreement
int check_agreement(Run& r) {
    const Options& o = r.opt;
    std::string err;
    if (o.compare_to.empty() != o.pair_agreement.empty()) return fail(o.compare_to.empty() ? "--pair-agreement needs --compare-to" : "--compare-to needs --pair-agreement");
    if (already_exists("Pair agreement", o.pair_agreement.text, err)) return fail(err);
    if (clashes({o.pair_agreement.text}, {o.pair_profile.text, o.pair_events.text, o.pair_stats.text, o.dist_out.text}, "--pair-agreement names the file of another output option", err))
        return fail(err);
    if (r.agreement() && r.cyclizes()) return fail("--compare-to and --pair-agreement cannot be combined with -c: the final graph then has cycles");
    return GO_ON;
}

// --msa-out / --column-stats / --variable-sites
int check_msa_columns(Run& r) {
    const Options& o = r.opt;
    std::string err;
    if (o.msa_layout.given && !r.msa_columns()) return fail("--msa-layout needs --msa-out, --column-stats or --variable-sites");
    if ((o.site_min_minor.given || o.site_max_gaps.given) && o.column_stats.empty() && o.variable_sites.empty())
        return fail(std::string(o.site_min_minor.given ? "--site-min-minor" : "--site-max-gaps") + " needs --column-stats or --variable-sites");
    if (o.msa_layout.given && (r.msa_layout = word_of(o.msa_layout, {"level", "node"})) < 0) return fail(expects("--msa-layout", "level or node", o.msa_layout));
    if (!take_whole(o.site_min_minor, 1, LLONG_MAX, r.site_min_minor)) return fail(expects("--site-min-minor", "a whole number of sequences, at least 1", o.site_min_minor));
    if (!take_whole(o.site_max_gaps, 0, LLONG_MAX, r.site_max_gaps)) return fail(expects("--site-max-gaps", "a whole number of sequences, at least 0", o.site_max_gaps));
    r.site_min_minor = std::min<uint64_t>(r.site_min_minor, 0xFFFFFFFFull);   // (more than any number of sequences either way)
    r.site_max_gaps = std::min<uint64_t>(r.site_max_gaps, 0xFFFFFFFFull);
    if (already_exists("MSA", o.msa_out.text, err) || already_exists("Column statistics", o.column_stats.text, err) || already_exists("Variable sites", o.variable_sites.text, err))
        return fail(err);
    if (!r.msa_columns()) return GO_ON;
    const std::vector<std::string> mine = {o.msa_out.text, o.column_stats.text, o.variable_sites.text};
    const std::vector<std::string> others = {o.pair_stats.text, o.dist_out.text, o.pair_profile.text, o.pair_events.text, o.pair_agreement.text, o.tree_out.text,
                                             r.config("subalignments_filepath")};
    for (size_t a = 0; a < mine.size(); ++a)
        if (clashes({mine[a]}, std::vector<std::string>(mine.begin() + a + 1, mine.end()), "--msa-out, --column-stats and --variable-sites must name different files", err) ||
            clashes({mine[a]}, others, "--msa-out, --column-stats and --variable-sites cannot name the file of another output option", err))
            return fail(err);
    if (r.cyclizes()) return fail("--msa-out, --column-stats and --variable-sites cannot be combined with -c: the final graph then has cycles");
    return GO_ON;
}

bool load_graph(const std::string& name, const char* what, NamedGraph& into, std::string& err) {
    std::string text;
    if (!read_input(name, text, err)) return false;
    if (!into.load(text.data(), text.size())) { err = std::string("cannot read the ") + what + " graph from " + name + ": not a GFA this tool writes"; return false; }
    if (const std::string* twice = into.repeated_name()) { err = std::string("the ") + what + " graph " + name + " has two paths named " + *twice; return false; }
    if (into.has_cycles()) { err = std::string("the ") + what + " graph " + name + " has cycles: a path meets a node twice"; return false; }
    return true;
}

// the baseline is read here: what is wrong with it needs no other input.  With --graph that is the run: no FASTA, no alignment, nothing on
// standard output, the given graph against the baseline
int load_graphs_and_compare(Run& r) {
    const Options& o = r.opt;
    std::string err;
    if (r.agreement()) {
        if (o.compare_to.text == "-" || o.graph.text == "-") return fail("--compare-to and --graph take files, not standard input");
        if (!load_graph(o.compare_to.text, "baseline", r.baseline, err)) return fail(err);
        if (o.graph.given && !load_graph(o.graph.text, "given", r.given, err)) return fail(err);
    }
    if (!o.graph.given) return GO_ON;
    g_level = atoi(r.config("logging_level").c_str());
    if (open_device(r) != GO_ON) return 1;
    if (!write_pair_agreement(r, r.given, err)) return fail(err);
    log_line(LOG_MINIMAL, "Compared " + o.graph.text + " with " + o.compare_to.text + ", exiting.");
    return 0;
}

int validate_config(Run& r) {
    // --dist-out alone passes the rows through a file of its own next to FILE, which must not be anybody else's
    if (!r.opt.dist_out.empty() && r.opt.pair_stats.empty()) r.dist_tmp = r.opt.dist_out.text + ".pair-stats.tmp";
    if (!r.dist_tmp.empty() && std::ifstream(r.dist_tmp).good()) return fail("--dist-out would overwrite " + r.dist_tmp + ": remove it or give --pair-stats");
    if (cl_config_validate(r.cfg)) return usage_error(r, lib_error());
    g_level = atoi(r.config("logging_level").c_str());
    std::string cmd = "Executing command:";
    for (int i = 0; i < r.argc; ++i) cmd += std::string(" ") + r.argv[i];
    log_line(LOG_MINIMAL, cmd);
    log_line(LOG_DEBUG, "config file:\n\n" + generate(r.cfg) + "\n");
    return GO_ON;
}

// the FASTA and the tree; the templates of --monomers-seed-period: pieces of the first sequence
int read_inputs(Run& r) {
    r.fasta_name = r.config("fasta_name");
    r.tree_name = r.config("tree_name");
    std::string err;
    if (!read_input(r.fasta_name, r.fasta_text, err)) return fail(err);
    if (!r.tree_name.empty() && !read_input(r.tree_name, r.newick, err)) return fail(err);
    log_line(LOG_BASIC, "Reading input.");
    if (!r.input.parse(r.fasta_text)) return fail(lib_error());
    const cl_fasta& fa = r.input.fa;
    r.n_sequences = fa.n_sequences;
    r.sequence_names.assign(fa.names, fa.names + fa.n_sequences);
    for (uint64_t i = 0; i < fa.n_sequences; ++i) r.n_bases += fa.lengths[i];
    if (r.seed_period) {
        cl_monomer_templates seeds;
        if (cl_monomer_seed_templates(fa.sequences, fa.lengths, fa.n_sequences, (uint32_t)r.seed_period, (uint32_t)r.seed_count, r.seed_start, r.monomers.strands, &seeds))
            return fail("--monomers-seed-period: " + lib_error());
        for (uint64_t m = 0; m < seeds.n_templates; ++m) r.templates.add(seeds.names[m], seeds.templates[m], seeds.lengths[m]);
        r.templates.point();
        cl_monomer_templates_free(&seeds);
    }
    for (const SequenceOutput& out : SEQUENCE_OUTPUTS)
        if (!(r.opt.*out.file).empty() && r.n_bases >= (1ull << 30))
            return fail(std::string(out.option) + " takes less than 2^30 bases, the input holds " + std::to_string(r.n_bases));
    return GO_ON;
}

std::string input_from(const Run& r) { return "FASTA input from " + (r.fasta_name == "-" ? std::string("STDIN") : r.fasta_name); }

// the sequence outputs: as the whole run (--x-only: the last of them first, no alignment, nothing on standard output) or on the way to the alignment
int write_sequence_outputs(Run& r, bool as_the_run) {
    for (int i = 0; i < 3; ++i) {
        const SequenceOutput& out = SEQUENCE_OUTPUTS[as_the_run ? 2 - i : i];
        const std::string& file = (r.opt.*out.file).text;
        if (as_the_run ? !(r.opt.*out.only).given : file.empty()) continue;
        if (as_the_run) {
            if (r.n_sequences < 1) return fail(input_from(r) + " contains no sequence");
            if (open_device(r) != GO_ON) return 1;
        } else {
            log_line(LOG_BASIC, std::string("Writing ") + out.what + ".");
        }
        std::string err;
        if (!out.write(r, err)) return fail(err);
        if (!as_the_run) continue;
        log_line(LOG_MINIMAL, std::string("Wrote ") + out.what + " to " + file + ", exiting.");
        return 0;
    }
    return GO_ON;
}

int run_only_outputs(Run& r) { return write_sequence_outputs(r, true); }

int check_sequence_counts(Run& r) {
    const bool printed_is_cigar = r.n_sequences == 2 && !r.opt.force_gfa_output.given;
    if (r.n_sequences < 2) return fail(input_from(r) + " contains " + std::to_string(r.n_sequences) + " sequence(s), cannot form an alignment");
    if (r.pair_positions() && printed_is_cigar) return fail("--pair-profile and --pair-events need --force-gfa-output for two sequences: they read the graph that is printed");
    if (r.agreement() && printed_is_cigar) return fail("--compare-to and --pair-agreement need --force-gfa-output for two sequences: they read the graph that is printed");
    if (r.msa_columns() && printed_is_cigar)
        return fail("--msa-out, --column-stats and --variable-sites need --force-gfa-output for two sequences: they read the graph that is printed");
    if (!r.opt.dist_out.empty()) {   // the rows name sequences as -A names its files: two names that differ only in '/' and '_' could not be told apart
        for (size_t a = 0; a < r.sequence_names.size(); ++a)
            for (size_t b = a + 1; b < r.sequence_names.size(); ++b)
                if (r.input.shown[a] == r.input.shown[b]) return fail("--dist-out cannot tell sequences " + r.sequence_names[a] + " and " + r.sequence_names[b] + " apart");
    }
    if (r.tree_name.empty() && !r.opt.infer_tree.given && r.refine_rounds == 0 && r.n_sequences > 2)
        fprintf(stderr, "warning: it is highly recommended to provide a guide tree (-T) when aligning > 2 sequences\n");
    return GO_ON;
}

// cl_msa's parameters; the device is opened only now: everything above works without one.  Then the sequence outputs on the way
int open_and_write_sequence_outputs(Run& r) {
    if (cl_config_msa_params(r.cfg, &r.mp)) return fail(lib_error());
    r.mp.force_gfa_output = r.opt.force_gfa_output.given;
    // --dist-out is computed from the rows of the --pair-stats file: without --pair-stats the run writes them next to FILE and the file is removed
    r.stats_file = !r.opt.pair_stats.empty() ? r.opt.pair_stats.text : r.dist_tmp;
    if (!r.stats_file.empty()) r.mp.pair_stats_path = r.stats_file.c_str();
    if (!r.devices.empty()) {
        r.mp.devices = r.devices.data();
        r.mp.n_devices = (int)r.devices.size();
    }
    log_line(LOG_VERBOSE, "Opening GPU " + std::to_string(r.devices.empty() ? 0 : r.devices[0]) + " with " + std::to_string(r.mp.n_workers) + " worker context(s).");
    if (open_device(r) != GO_ON) return 1;
    const int status = write_sequence_outputs(r, false);
    r.input.clear();
    return status;
}

// --infer-tree, --refine-tree, --tree-out: the tree goes to cl_msa exactly as the text of a -T file would
int make_guide_tree(Run& r) {
    r.have_tree = !r.tree_name.empty() || r.opt.infer_tree.given;
    std::string err;
    char line[128];
    if (r.opt.infer_tree.given) {
        log_line(LOG_BASIC, "Inferring a guide tree from k-mer distances.");
        const auto t0 = std::chrono::steady_clock::now();
        LibText tree;
        if (cl_infer_guide_tree(r.ctx, r.fasta_text.data(), r.fasta_text.size(), 21, &tree.text, &tree.len)) return fail(context_error(r.ctx));
        r.newick = tree.str();
        snprintf(line, sizeof(line), "Inferred the guide tree in %.3f s.", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        log_line(LOG_VERBOSE, line);
        log_line(LOG_DEBUG, "guide tree: " + r.newick);
    }
    if (r.refine_rounds > 0) {
        log_line(LOG_BASIC, "Refining the guide tree from alignment distances.");
        const auto t0 = std::chrono::steady_clock::now();
        int done = 0;
        // One round per call, so that each round's tree can be logged at -v 4: the same rounds, trees and convergence as one call with max_rounds = N
        // (a round depends on the tree text alone), at the price of parsing the FASTA once per round
        for (int i = 0; i < r.refine_rounds; ++i) {
            LibText tree;
            int rounds_run = 0, converged = 0;
            if (cl_refine_guide_tree(r.ctx, r.fasta_text.data(), r.fasta_text.size(), r.have_tree ? r.newick.c_str() : nullptr, &r.mp, 1, &tree.text, &tree.len, &rounds_run,
                                     &converged))
                return fail(context_error(r.ctx));
            if (tree.text) { r.newick = tree.str(); r.have_tree = true; }
            if (rounds_run == 0) break;   // fewer than three sequences: nothing to refine
            ++done;
            log_line(LOG_DEBUG, "guide tree after round " + std::to_string(done) + ": " + r.newick);
            if (converged) { log_line(LOG_VERBOSE, "The guide tree no longer changes."); break; }
        }
        snprintf(line, sizeof(line), "Refined the guide tree in %d round(s), %.3f s.", done, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        log_line(LOG_VERBOSE, line);
    }
    if (!r.opt.tree_out.empty() && !write_file(r.opt.tree_out.text, (r.have_tree ? r.newick : std::string()) + "\n", "the guide tree", err)) return fail(err);
    return GO_ON;
}

// cl_msa, its text to standard output, then the outputs that read the graph it printed
int align_and_write(Run& r) {
    log_line(LOG_BASIC, "Aligning " + std::to_string(r.n_sequences) + " sequences.");
    LibText text;
    if (cl_msa(r.ctx, r.fasta_text.data(), r.fasta_text.size(), r.have_tree ? r.newick.c_str() : nullptr, &r.mp, &text.text, &text.len, &r.st)) return fail(context_error(r.ctx));
    if (fwrite(text.text, 1, text.len, stdout) != text.len || fflush(stdout) != 0) return fail("could not write the alignment to standard output");
    if (!r.pair_positions() && !r.agreement() && !r.msa_columns()) return GO_ON;
    NamedGraph printed;
    std::string err;
    if (!printed.load(text.text, text.len)) return fail("cannot read back the alignment graph");
    if (r.pair_positions() && !write_pair_positions(r, printed, err)) return fail(err);
    if (r.agreement() && !write_pair_agreement(r, printed, err)) return fail(err);
    if (r.msa_columns() && !write_msa_columns(r, printed, err)) return fail(err);
    return GO_ON;
}

// --dist-out and the closing lines
int finish(Run& r) {
    if (!r.opt.dist_out.empty()) {
        std::string err;
        const bool ok = write_distances(r.stats_file, r.sequence_names, r.opt.dist_out.text, err);
        if (r.opt.pair_stats.empty()) remove(r.stats_file.c_str());
        if (!ok) return fail(err);
    }
    const cl_msa_stats& st = r.st;
    char line[512];
    snprintf(line, sizeof(line), "%llu merges, score scale %.6g: calibration %.2f s, matches %.2f s, alignment %.2f s, fusion %.2f s",
             (unsigned long long)st.n_merges, st.score_scale, st.calibration_s, st.match_s, st.align_s, st.fuse_s);
    log_line(LOG_VERBOSE, line);
    if (st.n_restarted) log_line(LOG_BASIC, "Loaded " + std::to_string(st.n_restarted) + " subproblem(s) from an earlier run.");
    if (r.mp.cyclize) log_line(LOG_BASIC, "Merged " + std::to_string(st.n_bonds) + " tandem duplication(s), realigned " + std::to_string(st.n_polished_regions) + " region(s).");
    snprintf(line, sizeof(line), "Run completed successfully in %.2f s, exiting.", st.total_s);
    log_line(LOG_MINIMAL, line);
    return 0;
}

// what happens, in order.  A stage returns GO_ON, or the exit status that ends the run
int run(int argc, char** argv) {
    Run r(argc, argv);
    if (!r.cfg || !r.defaults) return fail("out of memory");
    int (*const stages[])(Run&) = {
        parse_command_line,
        take_positional,
        generate_config,   // -G
        check_graph_alone,
        check_only_rule,
        load_config_file,   // -C
        check_dotplot,
        check_periods,
        check_monomers,
        check_tree_options,
        check_pair_outputs,
        check_agreement,
        check_msa_columns,
        load_graphs_and_compare,   // --graph ends here
        validate_config,
        read_inputs,
        run_only_outputs,   // --monomers-only, --periods-only and --dotplot-only end here
        check_sequence_counts,
        open_and_write_sequence_outputs,
        make_guide_tree,
        align_and_write,
        finish,
    };
    for (auto stage : stages) {
        const int status = stage(r);
        if (status != GO_ON) return status;
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        return run(argc, argv);
    } catch (const std::exception& e) {
        return fail(e.what());
    } catch (...) {
        return fail("unexpected failure");
    }
}
