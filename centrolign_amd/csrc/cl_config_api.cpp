// cl_config_api.cpp — the control plane: every parameter of the centrolign command line (src/parameters.cpp:12-108) with its name, type,
// group and the value the CLI starts from; the config-file text the reference reads (Parameters(std::istream&), :219-313) and writes
// (generate_config, :335-359); its bounds (validate, :362-463); and what apply (:112-194) hands to the pipeline, here a cl_msa_params.
// Host code only: nothing in this file touches a device.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "cl_internal.hpp"

namespace {

enum CfgType { T_INT, T_BOOL, T_DOUBLE, T_ENUM, T_STRING, T_DOUBLE3, T_INT3 };

struct CfgValue {
    int64_t i = 0;
    bool b = false;
    double d = 0.0;
    std::string s;
    double da[3] = {0, 0, 0};
    int64_t ia[3] = {0, 0, 0};
};

struct CfgParam {
    int group;
    const char* name;
    CfgType type;
    const char* deflt;   // the default as config text (parsed once, by the same parser a config file goes through)
    const char* help;    // comment lines of a generated config; '\n' separates lines
};

// the groups in the reference's order (Parameters::submodule_t)
const char* const kGroups[] = {
    "Input and output files, logging",
    "Finding matches between two graphs",
    "Chaining matches into anchors",
    "Telling alignable from unalignable regions",
    "Base-level alignment between anchors",
    "Merging tandem duplications into cycles",
    "Switches meant for development",
};

// every parameter of the reference's registry, in its order, with the values its CLI starts from
const CfgParam kParams[] = {
    {0, "fasta_name", T_STRING, "", "Input sequences (FASTA); '-' reads standard input"},
    {0, "tree_name", T_STRING, "", "Guide tree (Newick) whose leaf names are the FASTA's sequence names; empty: the sequences in file order"},
    {0, "logging_level", T_ENUM, "2", "How much progress goes to standard error:\n0 = nothing, 1 = minimal, 2 = basic, 3 = verbose, 4 = debug"},
    {0, "subproblems_prefix", T_STRING, "", "When set, the graph of every finished subproblem is written as GFA to files starting with this prefix"},
    {0, "restart", T_BOOL, "false", "Resume an interrupted run from the subproblem files under 'subproblems_prefix'"},
    {0, "all_pairs_prefix", T_STRING, "", "When set, the induced alignment of every pair of sequences is written as a CIGAR to files starting with this prefix"},
    {0, "subalignments_filepath", T_STRING, "", "When set, the path-to-path alignment of every merge is written to this file (it must not exist yet)"},
    {0, "threads", T_INT, "1", "Worker contexts that run calibrations and independent merges side by side"},

    {1, "max_count", T_INT, "3000", "Ignore matches that occur more often than this in either graph"},
    {1, "use_color_set_size", T_BOOL, "true", "Choice of the structure that counts match occurrences (no effect here: both give the same counts)"},

    {2, "max_num_match_pairs", T_INT, "1250000", "Budget of match pairs the chaining step considers per merge"},
    {2, "memory_restraint_size", T_INT, "1073741824", "Graph size times sequence count above which the reference switches to leaner chaining tables (no effect here)"},
    {2, "split_matches_at_branchpoints", T_BOOL, "true", "Cut matches where the graph forks so that chaining is not misled by reachability"},
    {2, "anchor_split_limit", T_INT, "5", "A cut is made only this close to the end of a match"},
    {2, "min_split_length", T_INT, "128", "Only matches at least this long are cut"},
    {2, "min_path_length_spread", T_INT, "50", "Only forks whose branches differ in length by at least this much cause a cut"},
    {2, "max_split_match_set_size", T_INT, "16", "Only matches shared by at most this many sequences are cut"},
    {2, "chaining_algorithm", T_ENUM, "2", "Chaining algorithm:\n0 = exhaustive (not offered here), 1 = sparse, 2 = sparse with affine gaps"},
    {2, "anchor_gap_open", T_DOUBLE3, "1.25,50,5000", "Piecewise gap open penalties of the affine chaining (increasing)"},
    {2, "anchor_gap_extend", T_DOUBLE3, "2.5,0.1,0.0015", "Piecewise gap extension penalties of the affine chaining (decreasing)"},
    {2, "anchor_score_function", T_ENUM, "2", "Weight of a match:\n0 = inverse count, 1 = length over count, 2 = concave length over count,\n"
                                               "3 = concave length minus count"},
    {2, "pair_count_power", T_DOUBLE, "0.5", "Exponent of the occurrence count in a match's weight"},
    {2, "length_intercept", T_DOUBLE, "2250", "Longest match that still weighs more than nothing (concave weights)"},
    {2, "length_decay_power", T_DOUBLE, "2", "Exponent of the length term subtracted in concave weights"},
    {2, "global_anchoring", T_BOOL, "true", "Chains span the whole sequences rather than local regions"},
    {2, "do_fill_in_anchoring", T_BOOL, "true", "Chain again inside the gaps of the chain with matches the budget left out"},

    {3, "constraint_method", T_ENUM, "3", "How the chain is cut into alignable and unalignable segments:\n"
                                           "0 = no cut, 1 = unconstrained, 2 = minimum average, 3 = minimum windowed average"},
    {3, "minimum_segment_score", T_DOUBLE, "15000", "Least total score of an alignable segment"},
    {3, "minimum_segment_average", T_DOUBLE, "0.1", "Least average score of an alignable segment"},
    {3, "window_length", T_DOUBLE, "10000", "Window of the windowed average"},
    {3, "generalized_length_mean", T_DOUBLE, "-0.5", "Exponent of the power mean that turns the two graphs' lengths into one"},
    {3, "boundary_score_factor", T_DOUBLE, "0.95", "Score a realignment's boundaries count with, as a share of the full score"},

    {4, "stitch_match", T_INT, "20", "Match score of the base-level alignment"},
    {4, "stitch_mismatch", T_INT, "80", "Mismatch penalty of the base-level alignment"},
    {4, "stitch_gap_open", T_INT3, "60,800,2500", "Piecewise gap open penalties of the base-level alignment (increasing)"},
    {4, "stitch_gap_extend", T_INT3, "30,5,1", "Piecewise gap extension penalties of the base-level alignment (decreasing)"},
    {4, "max_trivial_size", T_INT, "30000", "Largest matrix that is aligned even when its region was found unalignable"},
    {4, "min_wfa_size", T_INT, "40000000", "Smallest matrix handed to the graph wavefront aligner"},
    {4, "max_wfa_size", T_INT, "75000000", "Largest matrix handed to the graph wavefront aligner"},
    {4, "max_wfa_ratio", T_DOUBLE, "1.05", "Largest ratio of long to short side for the graph wavefront aligner"},
    {4, "wfa_pruning_dist", T_INT, "25", "How far a diagonal may lag before the wavefront aligner drops it"},
    {4, "deletion_alignment_ratio", T_INT, "8", "Least ratio of long to short side for the deletion aligner"},
    {4, "deletion_alignment_short_max_size", T_INT, "1500", "Longest short side for the deletion aligner"},
    {4, "deletion_alignment_long_min_size", T_INT, "2000", "Shortest long side for the deletion aligner"},
    {4, "indel_fuzz_score_proportion", T_DOUBLE, "0.001", "Anchors that pin a long indel are dropped when they carry at most this share of the score"},
    {4, "min_indel_fuzz_length", T_INT, "50", "Only indels at least this long are freed that way"},

    {5, "cyclize_tandem_duplications", T_BOOL, "false", "Find tandem duplications and merge them into cycles of the final graph"},
    {5, "max_tandem_duplication_search_rounds", T_INT, "3", "Most rounds of nested tandem duplications searched per sequence"},
    {5, "min_cyclizing_length", T_INT, "100000", "Shortest tandem duplication looked for"},
    {5, "tandem_dup_score_proportion", T_DOUBLE, "0.2", "Least score of a duplication's chain, as a share of the best chain over the same stretch"},
    {5, "include_tandem_dup_gap_scores", T_BOOL, "true", "Count gap scores into a duplication chain's score"},
    {5, "deviation_drift_factor", T_DOUBLE, "150", "Indel drift a duplication chain may show, times the square root of its length"},
    {5, "separation_drift_factor", T_DOUBLE, "50", "How close to the main diagonal a duplication chain may come, as length minus this times its square root"},
    {5, "trim_window_proportion", T_DOUBLE, "0.1", "Share of the length at either end used when trimming a duplication to its score"},
    {5, "deduplication_slosh_proportion", T_DOUBLE, "0.1", "Two duplications are one when they differ by at most this share of 'min_cyclizing_length'"},
    {5, "max_realignment_cycle_size", T_INT, "10000", "Cycles shorter than this are realigned after merging"},
    {5, "inconsistent_indel_window", T_INT, "100", "Largest distance between two indels that are realigned together"},
    {5, "min_inconsistency_disjoint_length", T_INT, "8", "Least disjoint unmerged sequence of two segments for a realignment"},
    {5, "min_inconsistency_total_length", T_INT, "50", "Least total unmerged sequence of two segments for a realignment"},
    {5, "realignment_min_padding", T_INT, "1000", "Padding sequence a realignment tries to take from every path"},
    {5, "realignment_max_padding", T_INT, "10000", "Padding stops before any path would add this much"},

    {6, "bonds_prefix", T_STRING, "", "When set, the alignment of every tandem duplication found is written to files starting with this prefix"},
    {6, "preserve_subproblems", T_BOOL, "false", "Keep the data of finished subproblems in memory (no effect here)"},
    {6, "skip_calibration", T_BOOL, "false", "Keep the starting score scale instead of calibrating it to the input's repetitiveness"},
};
constexpr size_t kNumParams = sizeof(kParams) / sizeof(kParams[0]);
constexpr int kNumGroups = sizeof(kGroups) / sizeof(kGroups[0]);

struct CfgError {
    std::string what;
};

[[noreturn]] void fail(const std::string& what) { throw CfgError{what}; }

int param_index(const std::string& name) {
    for (size_t k = 0; k < kNumParams; ++k)
        if (name == kParams[k].name) return (int)k;
    return -1;
}

// parse_int / parse_double / parse_bool (src/utility.cpp:66-96): stoll / stod must take the whole text
int64_t parse_int(const std::string& s) {
    errno = 0;
    char* end = nullptr;
    long long v = strtoll(s.c_str(), &end, 10);
    if (end == s.c_str() || errno == ERANGE || (size_t)(end - s.c_str()) != s.size()) fail("Could not parse \"" + s + "\" as an integer");
    return (int64_t)v;
}

double parse_double(const std::string& s) {
    errno = 0;
    char* end = nullptr;
    double v = strtod(s.c_str(), &end);
    if (end == s.c_str() || (errno == ERANGE && std::isinf(v)) || (size_t)(end - s.c_str()) != s.size())
        fail("Could not parse \"" + s + "\" as a decimal number");
    return v;
}

bool parse_bool(const std::string& s) {
    if (s == "true" || s == "True" || s == "TRUE" || s == "T" || s == "t" || s == "1") return true;
    if (s == "false" || s == "False" || s == "FALSE" || s == "F" || s == "f" || s == "0") return false;
    fail("Could not parse \"" + s + "\" as a Boolean value");
}

// tokenize (src/utility.cpp:98-111): a trailing delimiter adds no empty token
std::vector<std::string> tokenize(const std::string& s, char delim) {
    std::vector<std::string> out;
    size_t prev = 0;
    while (prev < s.size()) {
        size_t cur = s.find(delim, prev);
        if (cur == std::string::npos) cur = s.size();
        out.push_back(s.substr(prev, cur - prev));
        prev = cur + 1;
    }
    return out;
}

std::vector<std::string> parse_array3(const std::string& s) {
    auto t = tokenize(s, ',');
    if (t.size() != 3) fail("Expected 3 comma-separated values in input string '" + s + "'");
    return t;
}

// a double as config text: the shortest %g form from 6 significant digits up that reads back as the same number.  At 6 digits this is what
// the reference's value_str prints (a default-formatted stream); where 6 digits would lose the value, more are written
std::string format_double(double v) {
    char buf[64];
    for (int prec = 6; prec <= 17; ++prec) {
        snprintf(buf, sizeof(buf), "%.*g", prec, v);
        if (strtod(buf, nullptr) == v || std::isnan(v)) break;
    }
    return buf;
}

}  // namespace

struct cl_config {
    CfgValue v[kNumParams];
};

namespace {

void set_value(cl_config* c, size_t k, const std::string& text) {
    CfgValue& v = c->v[k];
    switch (kParams[k].type) {
    case T_INT:
    case T_ENUM: v.i = parse_int(text); break;
    case T_BOOL: v.b = parse_bool(text); break;
    case T_DOUBLE: v.d = parse_double(text); break;
    case T_STRING: v.s = text; break;
    case T_DOUBLE3: {
        auto t = parse_array3(text);
        double d[3];
        for (int i = 0; i < 3; ++i) d[i] = parse_double(t[i]);
        memcpy(v.da, d, sizeof(d));
        break;
    }
    case T_INT3: {
        auto t = parse_array3(text);
        int64_t a[3];
        for (int i = 0; i < 3; ++i) a[i] = parse_int(t[i]);
        memcpy(v.ia, a, sizeof(a));
        break;
    }
    }
}

std::string value_str(const cl_config* c, size_t k) {
    const CfgValue& v = c->v[k];
    switch (kParams[k].type) {
    case T_INT:
    case T_ENUM: return std::to_string(v.i);
    case T_BOOL: return v.b ? "true" : "false";
    case T_DOUBLE: return format_double(v.d);
    case T_STRING: return v.s;
    case T_DOUBLE3: return format_double(v.da[0]) + "," + format_double(v.da[1]) + "," + format_double(v.da[2]);
    case T_INT3: return std::to_string(v.ia[0]) + "," + std::to_string(v.ia[1]) + "," + std::to_string(v.ia[2]);
    }
    return std::string();
}

void fill_defaults(cl_config* c) {
    for (size_t k = 0; k < kNumParams; ++k) set_value(c, k, kParams[k].deflt);
}

size_t need(const char* name) {
    int k = param_index(name);
    if (k < 0) fail(std::string("No parameter with name ") + name);
    return (size_t)k;
}
int64_t geti(const cl_config* c, const char* name) { return c->v[need(name)].i; }
double getd(const cl_config* c, const char* name) { return c->v[need(name)].d; }
bool getb(const cl_config* c, const char* name) { return c->v[need(name)].b; }
const std::string& gets(const cl_config* c, const char* name) { return c->v[need(name)].s; }

// enforce_lim (include/centrolign/parameters.hpp): "Invalid value for parameter 'NAME', got V but expected a value >= L"
template <typename T>
void enforce(const cl_config* c, const char* name, bool lim_is_min, bool equal_ok, T lim) {
    const size_t k = need(name);
    const T value = std::is_floating_point<T>::value ? (T)c->v[k].d : (T)c->v[k].i;
    if ((value == lim && equal_ok) || (value > lim && lim_is_min) || (value < lim && !lim_is_min)) return;
    auto show = [](T x) { return std::is_floating_point<T>::value ? format_double((double)x) : std::to_string((int64_t)x); };
    fail(std::string("Invalid value for parameter '") + name + "', got " + show(value) + " but expected a value " + (lim_is_min ? ">" : "<") +
         (equal_ok ? "=" : "") + " " + show(lim));
}
template <typename T> void enforce_gt(const cl_config* c, const char* n, T l) { enforce<T>(c, n, true, false, l); }
template <typename T> void enforce_geq(const cl_config* c, const char* n, T l) { enforce<T>(c, n, true, true, l); }
template <typename T> void enforce_leq(const cl_config* c, const char* n, T l) { enforce<T>(c, n, false, true, l); }
template <typename T> void enforce_range(const cl_config* c, const char* n, T lo, T hi) { enforce_geq<T>(c, n, lo); enforce_leq<T>(c, n, hi); }

// Parameters::validate (src/parameters.cpp:362-463), in its order.  need_fasta: the check that an input is named (the one bound that
// cl_config_msa_params does not apply: the FASTA is the caller's business there)
void validate(const cl_config* c, bool need_fasta) {
    const int64_t i32max = std::numeric_limits<int32_t>::max();
    enforce_gt<int64_t>(c, "threads", 0);
    enforce_gt<int64_t>(c, "max_count", 0);
    enforce_gt<int64_t>(c, "max_num_match_pairs", 0);
    enforce_geq<int64_t>(c, "memory_restraint_size", 0);
    enforce_range<int64_t>(c, "anchor_score_function", 0, 3);
    enforce_gt<double>(c, "pair_count_power", 0.0);
    enforce_geq<double>(c, "length_intercept", 1.0);
    enforce_geq<double>(c, "length_decay_power", 0.0);
    enforce_geq<int64_t>(c, "anchor_split_limit", 0);
    enforce_geq<int64_t>(c, "min_path_length_spread", 0);
    enforce_geq<int64_t>(c, "min_split_length", 0);
    enforce_geq<int64_t>(c, "max_split_match_set_size", 0);
    enforce_range<int64_t>(c, "logging_level", 0, 4);
    enforce_range<int64_t>(c, "chaining_algorithm", 0, 2);
    enforce_range<int64_t>(c, "constraint_method", 0, 3);
    enforce_geq<double>(c, "minimum_segment_score", 0.0);
    enforce_geq<double>(c, "minimum_segment_average", 0.0);
    enforce_gt<double>(c, "window_length", 0.0);
    enforce_geq<double>(c, "boundary_score_factor", 0.0);
    enforce_range<int64_t>(c, "stitch_match", 0, i32max);
    enforce_range<int64_t>(c, "stitch_mismatch", 0, i32max);
    enforce_geq<int64_t>(c, "max_trivial_size", 0);
    enforce_geq<int64_t>(c, "min_wfa_size", 0);
    enforce_geq<int64_t>(c, "max_wfa_size", 0);
    enforce_geq<double>(c, "max_wfa_ratio", 1.0);
    enforce_geq<int64_t>(c, "wfa_pruning_dist", 0);
    enforce_geq<int64_t>(c, "deletion_alignment_ratio", 1);
    enforce_geq<int64_t>(c, "deletion_alignment_short_max_size", 0);
    enforce_geq<int64_t>(c, "deletion_alignment_long_min_size", 0);
    enforce_range<double>(c, "indel_fuzz_score_proportion", 0.0, 1.0);
    enforce_geq<int64_t>(c, "min_indel_fuzz_length", 0);
    if (getb(c, "cyclize_tandem_duplications")) enforce_gt<int64_t>(c, "max_tandem_duplication_search_rounds", 0);
    enforce_geq<int64_t>(c, "min_cyclizing_length", 0);
    enforce_range<double>(c, "tandem_dup_score_proportion", 0.0, 1.0);
    enforce_geq<double>(c, "deviation_drift_factor", 0.0);
    enforce_geq<double>(c, "separation_drift_factor", 0.0);
    enforce_geq<double>(c, "deduplication_slosh_proportion", 0.0);
    enforce_geq<double>(c, "trim_window_proportion", 0.0);
    enforce_geq<int64_t>(c, "max_realignment_cycle_size", 0);
    enforce_geq<int64_t>(c, "inconsistent_indel_window", 0);
    enforce_geq<int64_t>(c, "min_inconsistency_disjoint_length", 0);
    enforce_geq<int64_t>(c, "min_inconsistency_total_length", 0);
    enforce_geq<int64_t>(c, "realignment_min_padding", 0);
    enforce_geq<int64_t>(c, "realignment_max_padding", 0);
    if (getb(c, "restart") && gets(c, "subproblems_prefix").empty()) fail("Cannot restart mid-execution without setting 'subproblems_prefix'");
    if (need_fasta && gets(c, "fasta_name").empty()) fail("FASTA input is missing");
    if (geti(c, "max_wfa_size") < geti(c, "min_wfa_size"))
        fail("Got greater minimum than maximum for size of DP matrix for performing WFA: " + std::to_string(geti(c, "max_wfa_size")) + ", " +
             std::to_string(geti(c, "min_wfa_size")));
    const CfgValue& ago = c->v[need("anchor_gap_open")];
    const CfgValue& age = c->v[need("anchor_gap_extend")];
    for (int i = 1; i < 3; ++i)
        if (ago.da[i - 1] > ago.da[i] || age.da[i - 1] < age.da[i])
            fail("Anchor gap open penalties must be given in increasing order and gap extend penalties in decreasing order, got " +
                 value_str(c, need("anchor_gap_open")) + " and " + value_str(c, need("anchor_gap_extend")));
    for (int i = 0; i < 3; ++i) {
        if (ago.da[i] < 0) fail("Got negative anchoring gap open penalty " + format_double(ago.da[i]));
        if (age.da[i] < 0) fail("Got negative anchoring gap extend penalty " + format_double(age.da[i]));
    }
    const CfgValue& sgo = c->v[need("stitch_gap_open")];
    const CfgValue& sge = c->v[need("stitch_gap_extend")];
    for (int i = 1; i < 3; ++i)
        if (sgo.ia[i - 1] > sgo.ia[i] || sge.ia[i - 1] < sge.ia[i])
            fail("Stitching gap open penalties must be given in increasing order and gap extend penalties in decreasing order, got " +
                 value_str(c, need("stitch_gap_open")) + " and " + value_str(c, need("stitch_gap_extend")));
    for (int i = 0; i < 3; ++i) {
        if (sgo.ia[i] < 0) fail("Got negative stitching gap open penalty " + std::to_string(sgo.ia[i]));
        if (sgo.ia[i] > i32max) fail("Stitching gap open penalty must be less than " + std::to_string(i32max) + ", got " + std::to_string(sgo.ia[i]));
        if (sge.ia[i] < 0) fail("Got negative stitching gap extend penalty " + std::to_string(sge.ia[i]));
        if (sge.ia[i] > i32max) fail("Stitching gap extend penalty must be less than " + std::to_string(i32max) + ", got " + std::to_string(sge.ia[i]));
    }
}

// Parameters(std::istream&) (src/parameters.cpp:219-313): start from the defaults, skip up to and including the first "---", then
// "name: value" per line, '#' to the end of a line is a comment, a value may sit in double quotes
void parse_into(cl_config* c, std::string config) {
    const size_t delim = config.find("---");
    if (delim != std::string::npos) config = config.substr(delim + 3);
    size_t pos = 0;
    while (pos <= config.size()) {
        size_t eol = config.find('\n', pos);
        if (eol == std::string::npos) eol = config.size();
        const std::string line = config.substr(pos, eol - pos);
        pos = eol + 1;
        const size_t comment = line.find('#');
        const size_t end = comment == std::string::npos ? line.size() : comment;
        bool blank = true;
        for (size_t i = 0; i < end; ++i) blank = blank && isspace((unsigned char)line[i]);
        if (blank) continue;
        const size_t colon = line.find(':');
        if (colon == std::string::npos || colon >= end) fail("Config has line missing ':' delimiter in line '" + line + "'");
        size_t ns = 0, ne = colon, vs = colon + 1, ve = end;
        while (ns < ne && isspace((unsigned char)line[ns])) ++ns;
        while (ns < ne && isspace((unsigned char)line[ne - 1])) --ne;
        while (vs < ve && isspace((unsigned char)line[vs])) ++vs;
        while (vs < ve && isspace((unsigned char)line[ve - 1])) --ve;
        if (ns >= ne) fail("Config has line with no variable name in line '" + line + "'");
        if (vs >= ve) fail("Config has line with no variable value in line '" + line + "'");
        if (line[vs] == '"' && (ve == vs + 1 || line[ve - 1] != '"')) fail("Unmatched \" in config file line: " + line);
        if (line[vs] == '"') { ++vs; --ve; }
        const std::string name = line.substr(ns, ne - ns);
        set_value(c, need(name.c_str()), line.substr(vs, ve - vs));
    }
}

// Parameters::generate_config (src/parameters.cpp:335-359): the same keys, order, layout and quoting; the comments are this project's
std::string generate(const cl_config* c) {
    std::string out = "---\n";
    for (int g = 0; g < kNumGroups; ++g) {
        out += " \n ##########\n # ";
        out += kGroups[g];
        out += "\n ##########\n \n";
        for (size_t k = 0; k < kNumParams; ++k) {
            if (kParams[k].group != g) continue;
            for (const auto& h : tokenize(kParams[k].help, '\n')) out += " # " + h + "\n";
            const std::string v = value_str(c, k);
            bool ws = false;
            for (char ch : v) ws = ws || isspace((unsigned char)ch);
            const char* q = (ws || v.empty()) ? "\"" : "";
            out += std::string(" ") + kParams[k].name + ": " + q + v + q + "\n";
        }
    }
    return out;
}

char* dup_text(const std::string& s) {
    char* p = (char*)malloc(s.size() + 1);
    if (!p) fail("out of memory");
    memcpy(p, s.data(), s.size());
    p[s.size()] = 0;
    return p;
}

template <typename F>
int guarded(F&& body) {
    try {
        body();
        return CL_OK;
    } catch (const CfgError& e) {
        cl_set_error(nullptr, "%s", e.what.c_str());
        return CL_ERR_INVALID_ARGUMENT;
    } catch (const std::bad_alloc&) {
        cl_set_error(nullptr, "out of memory");
        return CL_ERR_OUT_OF_MEMORY;
    }
}

void copy_score_function(const cl_config* c, cl_chain_params* s) {
    const CfgValue& go = c->v[need("anchor_gap_open")];
    const CfgValue& ge = c->v[need("anchor_gap_extend")];
    for (int i = 0; i < 3; ++i) { s->gap_open[i] = go.da[i]; s->gap_extend[i] = ge.da[i]; }
    s->anchor_score_function = (int)geti(c, "anchor_score_function");
    s->pair_count_power = getd(c, "pair_count_power");
    s->length_intercept = getd(c, "length_intercept");
    s->length_decay_power = getd(c, "length_decay_power");
    s->global_anchoring = getb(c, "global_anchoring");
}

const char* c_str_or_null(const std::string& s) { return s.empty() ? nullptr : s.c_str(); }

}  // namespace

extern "C" {

cl_config* cl_config_default(void) {
    cl_config* c = nullptr;
    int rc = guarded([&] {
        c = new cl_config();
        fill_defaults(c);
    });
    if (rc) { delete c; return nullptr; }
    return c;
}

void cl_config_free(cl_config* cfg) { delete cfg; }

int cl_config_set(cl_config* cfg, const char* name, const char* text) {
    if (!cfg || !name || !text) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    return guarded([&] { set_value(cfg, need(name), text); });
}

int cl_config_get(const cl_config* cfg, const char* name, char** text_out) {
    if (!cfg || !name || !text_out) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    *text_out = nullptr;
    return guarded([&] { *text_out = dup_text(value_str(cfg, need(name))); });
}

int cl_config_parse(const char* text, uint64_t len, cl_config** out) {
    if (!out || (!text && len)) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    cl_config* c = nullptr;
    int rc = guarded([&] {
        c = new cl_config();
        fill_defaults(c);
        parse_into(c, std::string(text ? text : "", len));
    });
    if (rc) { delete c; return rc; }
    *out = c;
    return CL_OK;
}

int cl_config_generate(const cl_config* cfg, char** text_out, uint64_t* len_out) {
    if (!cfg || !text_out) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    *text_out = nullptr;
    return guarded([&] {
        const std::string s = generate(cfg);
        *text_out = dup_text(s);
        if (len_out) *len_out = s.size();
    });
}

int cl_config_validate(const cl_config* cfg) {
    if (!cfg) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    return guarded([&] { validate(cfg, true); });
}

int cl_config_msa_params(const cl_config* c, cl_msa_params* p) {
    if (!c || !p) { cl_set_error(nullptr, "null argument"); return CL_ERR_INVALID_ARGUMENT; }
    return guarded([&] {
        validate(c, false);
        cl_msa_params m;
        cl_msa_params_default(&m);
        // IO
        m.subproblems_prefix = c_str_or_null(gets(c, "subproblems_prefix"));
        m.restart = getb(c, "restart");
        m.induced_pairwise_prefix = c_str_or_null(gets(c, "all_pairs_prefix"));
        m.subalignments_path = c_str_or_null(gets(c, "subalignments_filepath"));
        const int64_t threads = geti(c, "threads");   // one worker is the struct's default (n_workers <= 1), kept as it spells it
        if (threads > 1) m.n_workers = (int)std::min<int64_t>(threads, std::numeric_limits<int>::max());
        // MatchFinding (use_color_set_size is carried, the match finder's counts do not depend on it)
        m.merge.match.max_count = (uint64_t)geti(c, "max_count");
        m.merge.match.use_color_set_size = getb(c, "use_color_set_size");
        // Anchoring: one ScoreFunction in the reference, read by the match filter, the chaining and the partition
        copy_score_function(c, &m.merge.match.score);
        copy_score_function(c, &m.merge.align.anchor.chain);
        copy_score_function(c, &m.merge.align.partition.score_function);
        m.merge.align.anchor.max_num_match_pairs = (uint64_t)geti(c, "max_num_match_pairs");
        m.merge.align.anchor.do_fill_in_anchoring = getb(c, "do_fill_in_anchoring");
        const int64_t algo = geti(c, "chaining_algorithm");
        m.merge.align.anchor.chaining_algorithm_plus_one = algo == 2 ? 0 : (int)algo + 1;   // 0 is the struct's spelling of the default
        m.merge.align.split_matches_at_branchpoints = getb(c, "split_matches_at_branchpoints");
        m.merge.align.split.anchor_split_limit = (uint64_t)geti(c, "anchor_split_limit");
        m.merge.align.split.min_split_length = (uint64_t)geti(c, "min_split_length");
        m.merge.align.split.min_path_length_spread = (uint64_t)geti(c, "min_path_length_spread");
        m.merge.align.split.max_split_match_set_size = (uint64_t)geti(c, "max_split_match_set_size");
        // IdentifyingAlignability
        m.merge.align.partition.constraint_method = (int)geti(c, "constraint_method");
        m.merge.align.partition.minimum_segment_score = getd(c, "minimum_segment_score");
        m.merge.align.partition.minimum_segment_average = getd(c, "minimum_segment_average");
        m.merge.align.partition.window_length = getd(c, "window_length");
        m.merge.align.partition.generalized_length_mean = getd(c, "generalized_length_mean");
        m.merge.align.partition.boundary_score_factor = getd(c, "boundary_score_factor");
        // Aligning
        cl_stitch_params& st = m.merge.align.stitch;
        st.alignment_params.match = (uint32_t)geti(c, "stitch_match");
        st.alignment_params.mismatch = (uint32_t)geti(c, "stitch_mismatch");
        const CfgValue& sgo = c->v[need("stitch_gap_open")];
        const CfgValue& sge = c->v[need("stitch_gap_extend")];
        for (int i = 0; i < 3; ++i) { st.alignment_params.gap_open[i] = (uint32_t)sgo.ia[i]; st.alignment_params.gap_extend[i] = (uint32_t)sge.ia[i]; }
        st.max_trivial_size = (uint64_t)geti(c, "max_trivial_size");
        st.min_wfa_size = (uint64_t)geti(c, "min_wfa_size");
        st.max_wfa_size = (uint64_t)geti(c, "max_wfa_size");
        st.max_wfa_ratio = getd(c, "max_wfa_ratio");
        st.wfa_pruning_dist = (uint64_t)geti(c, "wfa_pruning_dist");
        st.deletion_alignment_ratio = (uint64_t)geti(c, "deletion_alignment_ratio");
        st.deletion_alignment_short_max_size = (uint64_t)geti(c, "deletion_alignment_short_max_size");
        st.deletion_alignment_long_min_size = (uint64_t)geti(c, "deletion_alignment_long_min_size");
        m.merge.align.indel_fuzz_score_proportion = getd(c, "indel_fuzz_score_proportion");
        m.merge.align.min_indel_fuzz_length = geti(c, "min_indel_fuzz_length");
        // InducingCycles
        m.cyclize = getb(c, "cyclize_tandem_duplications");
        m.max_tandem_duplication_search_rounds = (uint64_t)geti(c, "max_tandem_duplication_search_rounds");
        m.bonds.min_length = (double)geti(c, "min_cyclizing_length");
        m.bonds.min_opt_proportion = getd(c, "tandem_dup_score_proportion");
        m.bonds.include_gap_scores = getb(c, "include_tandem_dup_gap_scores");
        m.bonds.deviation_drift_factor = getd(c, "deviation_drift_factor");
        m.bonds.separation_drift_factor = getd(c, "separation_drift_factor");
        m.bonds.deduplication_slosh_proportion = getd(c, "deduplication_slosh_proportion");
        m.bonds.trim_window_proportion = getd(c, "trim_window_proportion");
        m.polish.max_tight_cycle_size = (uint64_t)geti(c, "max_realignment_cycle_size");
        m.polish.max_bond_inconsistency_window = (uint64_t)geti(c, "inconsistent_indel_window");
        m.polish.min_inconsistency_disjoint_length = (uint64_t)geti(c, "min_inconsistency_disjoint_length");
        m.polish.min_inconsistency_total_length = (uint64_t)geti(c, "min_inconsistency_total_length");
        m.polish.padding_target_min_length = (uint64_t)geti(c, "realignment_min_padding");
        m.polish.padding_max_length_limit = (uint64_t)geti(c, "realignment_max_padding");
        // DeveloperTools (preserve_subproblems: finished subproblems are not kept here either way)
        m.bonds_prefix = c_str_or_null(gets(c, "bonds_prefix"));
        m.skip_calibration = getb(c, "skip_calibration");
        *p = m;
    });
}

}  // extern "C"
