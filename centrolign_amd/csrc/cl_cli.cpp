// cl_cli.cpp — the `centrolign` executable: the reference's command line (src/main.cpp) over the library's C ABI.  Options and their
// order of effect are the reference's; the parameters live in a cl_config (cl_config_api.cpp) and the run is one cl_msa call.
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
#include <cmath>
#include <chrono>
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

int fail(const std::string& msg) {
    fprintf(stderr, "error: %s\n", msg.c_str());
    return 1;
}

std::string config_value(const cl_config* cfg, const char* name) {
    char* t = nullptr;
    if (cl_config_get(cfg, name, &t)) return std::string();
    std::string s(t);
    free(t);
    return s;
}

std::string generate(const cl_config* cfg) {
    char* t = nullptr;
    uint64_t n = 0;
    if (cl_config_generate(cfg, &t, &n)) return std::string();
    std::string s(t, n);
    free(t);
    return s;
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

bool parse_devices(const char* text, std::vector<int>& out) {
    std::string s(text);
    size_t pos = 0;
    while (pos <= s.size()) {
        size_t comma = s.find(',', pos);
        if (comma == std::string::npos) comma = s.size();
        const std::string tok = s.substr(pos, comma - pos);
        char* end = nullptr;
        errno = 0;
        long v = strtol(tok.c_str(), &end, 10);
        if (tok.empty() || *end || errno || v < 0 || v > 1 << 20) return false;
        out.push_back((int)v);
        pos = comma + 1;
    }
    return !out.empty();
}

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
        std::string nm = names[q];
        for (char& c : nm) if (c == '/') c = '_';
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
    std::ofstream out(dist_file, std::ios::binary);
    if (out) out.write(text.data(), (std::streamsize)text.size());
    out.close();
    if (!out) { err = "could not write the distance matrix to " + dist_file; return false; }
    return true;
}

// a whole number >= 1 (--window, --min-event)
bool parse_positive(const std::string& text, uint64_t& out) {
    if (text.empty() || text.size() > 18) return false;
    for (char c : text) if (c < '0' || c > '9') return false;
    out = strtoull(text.c_str(), nullptr, 10);
    return out >= 1;
}

// --pair-profile / --pair-events: the GFA text the run printed is read back (cl_read_gfa, as cl_refine_guide_tree does) and every pair (p, q), p < q,
// of its paths goes through the batch entry points; names as --pair-stats writes them
bool write_pair_positions(cl_context* ctx, const char* gfa, uint64_t gfa_len, const std::string& profile_file, uint64_t window, const std::string& events_file,
                          uint64_t min_event, std::string& err) {
    cl_owned_base_graph* owned = nullptr;
    char** path_names = nullptr;
    uint64_t n_paths = 0;
    if (cl_read_gfa(gfa, gfa_len, 1, &owned, &path_names, &n_paths)) { err = "cannot read back the alignment graph"; return false; }
    struct FreeGraph { cl_owned_base_graph* g; ~FreeGraph() { cl_owned_base_graph_free(g); } } free_graph{owned};
    std::vector<std::string> names;
    for (uint64_t p = 0; p < n_paths; ++p) {
        names.emplace_back(path_names[p]);
        for (char& c : names.back()) if (c == '/') c = '_';
        free(path_names[p]);
    }
    free(path_names);
    cl_base_graph g;
    cl_owned_base_graph_view(owned, &g);
    std::vector<uint64_t> pairs;
    for (uint64_t p = 0; p < n_paths; ++p)
        for (uint64_t q = p + 1; q < n_paths; ++q) { pairs.push_back(p); pairs.push_back(q); }
    const uint64_t n_pairs = pairs.size() / 2;
    std::vector<uint64_t> off(n_pairs + 1);
    auto lib_failure = [&](const char* what) {
        const char* e = cl_last_error(ctx);
        err = std::string(what) + ": " + (e && *e ? e : "failed");
        return false;
    };
    auto write_file = [&](const std::string& name, const std::string& text) {
        std::ofstream out(name, std::ios::binary);
        if (out) out.write(text.data(), (std::streamsize)text.size());
        out.close();
        if (!out) err = "could not write to " + name;
        return (bool)out;
    };
    if (!profile_file.empty()) {
        cl_pair_window* win = nullptr;
        if (cl_induced_pairwise_profiles(ctx, &g, pairs.data(), n_pairs, window, &win, off.data())) return lib_failure("pairwise profiles of the alignment graph");
        std::string tsv = "sample1\tsample2\twindow_start\twindow_end\tmatches\tmismatches\tinsertions\tdeletions\n";
        for (uint64_t k = 0; k < n_pairs; ++k) {
            const uint64_t n1 = g.path_off[pairs[2 * k] + 1] - g.path_off[pairs[2 * k]];
            const std::string lead = names[pairs[2 * k]] + "\t" + names[pairs[2 * k + 1]];
            for (uint64_t w = 0; w < off[k + 1] - off[k]; ++w) {
                const cl_pair_window& c = win[off[k] + w];
                char num[160];
                snprintf(num, sizeof(num), "\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)std::min(w * window, n1),
                         (unsigned long long)std::min((w + 1) * window, n1), (unsigned long long)c.eq, (unsigned long long)c.x, (unsigned long long)c.ins,
                         (unsigned long long)c.del);
                tsv += lead;
                tsv += num;
            }
        }
        free(win);
        if (!write_file(profile_file, tsv)) return false;
    }
    if (!events_file.empty()) {
        cl_gap_event* ev = nullptr;
        if (cl_induced_gap_events_batch(ctx, &g, pairs.data(), n_pairs, min_event, &ev, off.data())) return lib_failure("gap events of the alignment graph");
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
        if (!write_file(events_file, tsv)) return false;
    }
    return true;
}

// a whole number >= 0 (--site-max-gaps)
bool parse_count(const std::string& text, uint64_t& out) {
    if (text.empty() || text.size() > 18) return false;
    for (char c : text) if (c < '0' || c > '9') return false;
    out = strtoull(text.c_str(), nullptr, 10);
    return true;
}

// --msa-out / --column-stats / --variable-sites: the GFA text the run printed is read back (cl_read_gfa, as above) and goes through one
// cl_msa_columns_compute call that makes what the files named need; entries in the printed graph's path order under the paths' names
bool write_msa_columns(cl_context* ctx, const char* gfa, uint64_t gfa_len, const std::string& msa_file, const std::string& stats_file, const std::string& sites_file,
                       int layout, uint32_t min_minor, uint32_t max_gaps, std::string& err) {
    cl_owned_base_graph* owned = nullptr;
    char** path_names = nullptr;
    uint64_t n_paths = 0;
    if (cl_read_gfa(gfa, gfa_len, 1, &owned, &path_names, &n_paths)) { err = "cannot read back the alignment graph"; return false; }
    struct FreeGraph { cl_owned_base_graph* g; ~FreeGraph() { cl_owned_base_graph_free(g); } } free_graph{owned};
    std::vector<std::string> names;
    for (uint64_t p = 0; p < n_paths; ++p) { names.emplace_back(path_names[p]); free(path_names[p]); }
    free(path_names);
    cl_base_graph g;
    cl_owned_base_graph_view(owned, &g);
    cl_msa_columns_params params;
    cl_msa_columns_params_default(&params);
    params.layout = layout;
    params.want = (msa_file.empty() ? 0u : 1u) | (stats_file.empty() ? 0u : 2u) | (sites_file.empty() ? 0u : 4u);
    params.min_minor = min_minor;
    params.max_gaps = max_gaps;
    const auto t0 = std::chrono::steady_clock::now();
    cl_msa_columns m;
    if (cl_msa_columns_compute(ctx, &g, &params, &m)) {
        const char* e = cl_last_error(ctx);
        err = std::string("the alignment graph as columns: ") + (e && *e ? e : "failed");
        return false;
    }
    struct FreeColumns { cl_msa_columns* m; ~FreeColumns() { cl_msa_columns_free(m); } } free_columns{&m};
    {
        char line[200];
        snprintf(line, sizeof(line), "The alignment as columns (%s layout): %llu column(s)%s in %.3f s.", layout == 0 ? "level" : "node", (unsigned long long)m.n_cols,
                 sites_file.empty() ? "" : (", " + std::to_string(m.n_sites) + " variable site(s)").c_str(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        log_line(LOG_VERBOSE, line);
    }
    auto write_file = [&](const std::string& name, const std::string& text) {
        std::ofstream out(name, std::ios::binary);
        if (out) out.write(text.data(), (std::streamsize)text.size());
        out.close();
        if (!out) err = "could not write to " + name;
        return (bool)out;
    };
    auto fasta = [&](const char* rows, uint64_t width) {
        std::string text;
        for (uint64_t p = 0; p < n_paths; ++p) {
            text += '>'; text += names[p]; text += '\n';
            text.append(rows + p * width, width);
            text += '\n';
        }
        return text;
    };
    if (!msa_file.empty() && !write_file(msa_file, fasta(m.rows, m.n_cols))) return false;
    if (!stats_file.empty()) {
        std::string tsv = "column\tA\tC\tG\tT\tN\tgaps\tconsensus\tsite\n";
        for (uint64_t c = 0; c < m.n_cols; ++c) {
            const cl_msa_column& r = m.columns[c];
            char num[160];
            snprintf(num, sizeof(num), "%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%c\t%u\n", (unsigned long long)c, r.count[0], r.count[1], r.count[2], r.count[3], r.count[4], r.gaps,
                     "ACGTN-"[r.consensus], r.flags & 1u);
            tsv += num;
        }
        if (!write_file(stats_file, tsv)) return false;
    }
    if (!sites_file.empty() && !write_file(sites_file, fasta(m.site_rows, m.n_sites))) return false;
    return true;
}

// a GFA text as the graph the comparisons read (cl_read_gfa, as above) with its path names
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

// --compare-to / --pair-agreement: every pair (p, q), p < q, of the printed graph's paths against the same two sequences in the baseline, found there
// by name; names as --pair-stats writes them.  The baseline is graph a of cl_induced_pairwise_agreements: aligned_base, matches_base are its columns
bool write_pair_agreement(cl_context* ctx, const NamedGraph& printed, const NamedGraph& base, const std::string& file, std::string& err) {
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
    if (cl_induced_pairwise_agreements(ctx, &base.g, &printed.g, quads.data(), n_quads, got.data())) {
        const char* e = cl_last_error(ctx);
        err = std::string("agreement with the baseline graph: ") + (e && *e ? e : "failed");
        return false;
    }
    std::string tsv = "sample1\tsample2\taligned_base\taligned\tshared\tmatches_base\tmatches\tshared_matches\n";
    uint64_t aligned_base = 0, aligned = 0, shared = 0;
    for (uint64_t k = 0; k < n_quads; ++k) {
        std::string lead = printed.names[quads[4 * k + 2]] + "\t" + printed.names[quads[4 * k + 3]];
        for (char& c : lead) if (c == '/') c = '_';
        const cl_pair_agreement& r = got[k];
        char num[200];
        snprintf(num, sizeof(num), "\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)r.aligned_a, (unsigned long long)r.aligned_b,
                 (unsigned long long)r.shared, (unsigned long long)r.eq_a, (unsigned long long)r.eq_b, (unsigned long long)r.shared_eq);
        tsv += lead;
        tsv += num;
        aligned_base += r.aligned_a; aligned += r.aligned_b; shared += r.shared;
    }
    std::ofstream out(file, std::ios::binary);
    if (out) out.write(tsv.data(), (std::streamsize)tsv.size());
    out.close();
    if (!out) { err = "could not write to " + file; return false; }
    char line[256];
    snprintf(line, sizeof(line), "Agreement with the baseline over %llu pair(s): recall %.6f (%llu shared of %llu aligned there), precision %.6f (of %llu aligned here).",
             (unsigned long long)n_quads, aligned_base ? (double)shared / (double)aligned_base : 1.0, (unsigned long long)shared, (unsigned long long)aligned_base,
             aligned ? (double)shared / (double)aligned : 1.0, (unsigned long long)aligned);
    log_line(LOG_BASIC, line);
    return true;
}

// --dotplot: the windowed k-mer identity map of the FASTA's sequences, named as --pair-stats names them
bool write_dotplot(cl_context* ctx, const std::string& fasta_text, const cl_dotplot_params& params, const std::string& file, std::string& err) {
    cl_fasta fa;
    if (cl_parse_fasta(nullptr, fasta_text.data(), fasta_text.size(), &fa)) { err = lib_error(); return false; }
    struct FreeFasta { cl_fasta* f; ~FreeFasta() { cl_fasta_free(f); } } free_fasta{&fa};
    std::vector<std::string> shown(fa.names, fa.names + fa.n_sequences);
    std::vector<const char*> names;
    for (std::string& nm : shown) { std::replace(nm.begin(), nm.end(), '/', '_'); names.push_back(nm.c_str()); }
    cl_dotplot plot;
    if (cl_kmer_dotplot_compute(ctx, fa.sequences, fa.lengths, fa.n_sequences, &params, &plot)) {
        const char* e = cl_last_error(ctx);
        err = std::string("the dot plot: ") + (e && *e ? e : "failed");
        return false;
    }
    struct FreePlot { cl_dotplot* d; ~FreePlot() { cl_dotplot_free(d); } } free_plot{&plot};
    char line[256];
    snprintf(line, sizeof(line), "The dot plot: %llu windows of %u bases, %llu entries; k-mer lists %.3f ms, window pairs %.3f ms on the device.",
             (unsigned long long)plot.n_windows, plot.window, (unsigned long long)plot.n_entries, plot.spectra_ms, plot.pairs_ms);
    log_line(LOG_VERBOSE, line);
    char* text = nullptr;
    uint64_t len = 0;
    if (cl_dotplot_tsv(&plot, names.data(), fa.lengths, &text, &len)) { err = "the dot plot: " + lib_error(); return false; }
    FILE* f = fopen(file.c_str(), "wb");
    const bool written = f && fwrite(text, 1, len, f) == len;
    free(text);
    if ((f && fclose(f) != 0) || !written) { err = "could not write the dot plot to " + file; return false; }
    return true;
}

// --periods / --periods-hist: the repeat period spectra of the FASTA's sequences, named as --pair-stats names them
bool write_periods(cl_context* ctx, const std::string& fasta_text, const cl_periods_params& params, int scope, const std::string& file, const std::string& hist_file,
                   std::string& err) {
    cl_fasta fa;
    if (cl_parse_fasta(nullptr, fasta_text.data(), fasta_text.size(), &fa)) { err = lib_error(); return false; }
    struct FreeFasta { cl_fasta* f; ~FreeFasta() { cl_fasta_free(f); } } free_fasta{&fa};
    std::vector<std::string> shown(fa.names, fa.names + fa.n_sequences);
    std::vector<const char*> names;
    for (std::string& nm : shown) { std::replace(nm.begin(), nm.end(), '/', '_'); names.push_back(nm.c_str()); }
    cl_period_spectrum spec;
    if (cl_period_spectrum_compute(ctx, fa.sequences, fa.lengths, fa.n_sequences, &params, &spec)) {
        const char* e = cl_last_error(ctx);
        err = std::string("the period spectra: ") + (e && *e ? e : "failed");
        return false;
    }
    struct FreeSpectrum { cl_period_spectrum* d; ~FreeSpectrum() { cl_period_spectrum_free(d); } } free_spectrum{&spec};
    uint64_t n_links = 0;
    for (uint64_t s = 0; s < spec.n_seq; ++s) n_links += spec.links[spec.n_windows + s];
    char line[256];
    snprintf(line, sizeof(line), "The period spectra: %llu rows of %u bins, %llu links; links %.3f ms, histograms %.3f ms on the device.",
             (unsigned long long)spec.n_rows, spec.max_period + 1, (unsigned long long)n_links, spec.links_ms, spec.hist_ms);
    log_line(LOG_VERBOSE, line);
    for (int which = 0; which < 2; ++which) {
        const std::string& to = which == 0 ? file : hist_file;
        if (to.empty()) continue;
        char* text = nullptr;
        uint64_t len = 0;
        if ((which == 0 ? cl_periods_tsv : cl_periods_hist_tsv)(&spec, names.data(), fa.lengths, scope, &text, &len)) { err = "the period spectra: " + lib_error(); return false; }
        FILE* f = fopen(to.c_str(), "wb");
        const bool written = f && fwrite(text, 1, len, f) == len;
        free(text);
        if ((f && fclose(f) != 0) || !written) { err = "could not write the period spectra to " + to; return false; }
    }
    return true;
}

// --monomers / --monomers-summary: the monomer decomposition of the FASTA's sequences, named as --pair-stats names them
struct MonomerTemplates {
    std::vector<std::string> names, bases;
    std::vector<const char*> name_ptr, base_ptr;
    std::vector<uint64_t> lengths;
};

// the templates of --monomers-templates, held to the library's limits (host only)
bool read_monomer_templates(const std::string& file, int strands, MonomerTemplates& t, std::string& err) {
    std::string text;
    {
        std::ifstream in(file, std::ios::binary);
        if (!in) { err = "--monomers-templates: cannot open " + file; return false; }
        text.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    }
    cl_fasta fa;
    if (cl_parse_fasta(nullptr, text.data(), text.size(), &fa)) { err = "--monomers-templates " + file + ": " + lib_error(); return false; }
    struct FreeFasta { cl_fasta* f; ~FreeFasta() { cl_fasta_free(f); } } free_fasta{&fa};
    if (fa.n_sequences < 1) { err = "--monomers-templates " + file + " holds no template"; return false; }
    uint64_t total = 0;
    for (uint64_t m = 0; m < fa.n_sequences; ++m) {
        if (fa.lengths[m] < 1 || fa.lengths[m] > 1024) {
            err = "--monomers-templates: template " + std::string(fa.names[m]) + " has " + std::to_string(fa.lengths[m]) + " bases, not 1 to 1024";
            return false;
        }
        total += fa.lengths[m] * (uint64_t)strands;
        t.names.push_back(fa.names[m]);
        t.bases.push_back(std::string(fa.sequences[m], fa.lengths[m]));
        t.lengths.push_back(fa.lengths[m]);
    }
    if (total > 8192) { err = "--monomers-templates: " + std::to_string(total) + " template bases in all (both strands counted), more than 8192"; return false; }
    for (size_t m = 0; m < t.names.size(); ++m) { t.name_ptr.push_back(t.names[m].c_str()); t.base_ptr.push_back(t.bases[m].c_str()); }
    return true;
}

// --monomers-rounds, --monomers-least-share, --monomers-write-templates, --monomers-pileup
struct MonomerRefinement {
    uint32_t rounds = 0, least_share = 0;
    std::string templates_file, pileup_file;
};

bool write_text_file(const std::string& to, const char* text, uint64_t len) {
    FILE* f = fopen(to.c_str(), "wb");
    const bool written = f && fwrite(text, 1, len, f) == len;
    return !((f && fclose(f) != 0) || !written);
}

bool write_monomers(cl_context* ctx, const std::string& fasta_text, const MonomerTemplates& given, const cl_monomers_params& params, const MonomerRefinement& refinement,
                    const std::string& file, const std::string& summary_file, std::string& err) {
    cl_fasta fa;
    if (cl_parse_fasta(nullptr, fasta_text.data(), fasta_text.size(), &fa)) { err = lib_error(); return false; }
    struct FreeFasta { cl_fasta* f; ~FreeFasta() { cl_fasta_free(f); } } free_fasta{&fa};
    std::vector<std::string> shown(fa.names, fa.names + fa.n_sequences);
    std::vector<const char*> names;
    for (std::string& nm : shown) { std::replace(nm.begin(), nm.end(), '/', '_'); names.push_back(nm.c_str()); }
    MonomerTemplates t = given;   // the final templates: the given ones unless rounds are asked for
    char line[320];
    if (refinement.rounds) {
        cl_monomer_templates refined;
        if (cl_monomer_templates_refine_compute(ctx, fa.sequences, fa.lengths, fa.n_sequences, given.base_ptr.data(), given.lengths.data(), given.lengths.size(), &params,
                                                refinement.least_share, refinement.rounds, &refined)) {
            const char* e = cl_last_error(ctx);
            err = std::string("the template refinement: ") + (e && *e ? e : "failed");
            return false;
        }
        for (uint32_t r = 0; r < refined.rounds; ++r) {
            const cl_monomer_round& q = refined.round[r];
            snprintf(line, sizeof(line), "Template round %u: %llu blocks, %llu used, %llu templates changed; rows %.3f ms, blocks %.3f ms, alignments %.3f ms, counts %.3f ms on the device.",
                     r + 1, (unsigned long long)q.blocks, (unsigned long long)q.used, (unsigned long long)q.changed, q.dp_ms, q.trace_ms, q.align_ms, q.count_ms);
            log_line(LOG_VERBOSE, line);
        }
        snprintf(line, sizeof(line), "The templates %s after %u round(s).", refined.converged ? "converged" : "did not converge", refined.rounds);
        log_line(LOG_VERBOSE, line);
        for (size_t m = 0; m < t.bases.size(); ++m) { t.bases[m].assign(refined.templates[m], refined.lengths[m]); t.lengths[m] = refined.lengths[m]; }
        cl_monomer_templates_free(&refined);
    }
    t.name_ptr.clear();
    t.base_ptr.clear();
    for (size_t m = 0; m < t.names.size(); ++m) { t.name_ptr.push_back(t.names[m].c_str()); t.base_ptr.push_back(t.bases[m].c_str()); }
    if (!refinement.templates_file.empty()) {
        char* text = nullptr;
        uint64_t len = 0;
        if (cl_monomer_templates_fasta(t.name_ptr.data(), t.base_ptr.data(), t.lengths.data(), t.lengths.size(), &text, &len)) { err = "the templates: " + lib_error(); return false; }
        const bool written = write_text_file(refinement.templates_file, text, len);
        free(text);
        if (!written) { err = "could not write the templates to " + refinement.templates_file; return false; }
    }
    cl_monomer_decomposition dec;
    if (cl_monomer_decompose_compute(ctx, fa.sequences, fa.lengths, fa.n_sequences, t.base_ptr.data(), t.lengths.data(), t.lengths.size(), &params, &dec)) {
        const char* e = cl_last_error(ctx);
        err = std::string("the monomer decomposition: ") + (e && *e ? e : "failed");
        return false;
    }
    struct FreeDecomposition { cl_monomer_decomposition* d; ~FreeDecomposition() { cl_monomer_decomposition_free(d); } } free_decomposition{&dec};
    snprintf(line, sizeof(line), "The monomer decomposition: %llu problems, %llu blocks; rows %.3f ms, blocks %.3f ms on the device.",
             (unsigned long long)dec.n_problems, (unsigned long long)dec.n_blocks, dec.dp_ms, dec.trace_ms);
    log_line(LOG_VERBOSE, line);
    if (!refinement.pileup_file.empty()) {
        cl_monomer_pileup pile;
        if (cl_monomer_pileup_compute(ctx, fa.sequences, fa.lengths, fa.n_sequences, t.base_ptr.data(), t.lengths.data(), t.lengths.size(), &params, &dec,
                                      refinement.least_share, &pile)) {
            const char* e = cl_last_error(ctx);
            err = std::string("the monomer pileup: ") + (e && *e ? e : "failed");
            return false;
        }
        uint64_t used = 0;
        for (uint64_t m = 0; m < pile.n_templates; ++m) used += pile.used[m];
        snprintf(line, sizeof(line), "The monomer pileup: %llu blocks used; alignments %.3f ms, counts %.3f ms on the device.", (unsigned long long)used, pile.align_ms,
                 pile.count_ms);
        log_line(LOG_VERBOSE, line);
        char* text = nullptr;
        uint64_t len = 0;
        const int rc = cl_monomer_pileup_tsv(&pile, t.name_ptr.data(), t.base_ptr.data(), t.lengths.data(), t.lengths.size(), &text, &len);
        cl_monomer_pileup_free(&pile);
        if (rc) { err = "the monomer pileup: " + lib_error(); return false; }
        const bool written = write_text_file(refinement.pileup_file, text, len);
        free(text);
        if (!written) { err = "could not write the monomer pileup to " + refinement.pileup_file; return false; }
    }
    for (int which = 0; which < 2; ++which) {
        const std::string& to = which == 0 ? file : summary_file;
        if (to.empty()) continue;
        char* text = nullptr;
        uint64_t len = 0;
        if ((which == 0 ? cl_monomers_tsv : cl_monomers_summary_tsv)(&dec, names.data(), t.name_ptr.data(), t.lengths.data(), t.lengths.size(), &params, &text, &len)) {
            err = "the monomer decomposition: " + lib_error();
            return false;
        }
        FILE* f = fopen(to.c_str(), "wb");
        const bool written = f && fwrite(text, 1, len, f) == len;
        free(text);
        if ((f && fclose(f) != 0) || !written) { err = "could not write the monomer decomposition to " + to; return false; }
    }
    return true;
}

void print_help(const cl_config* defaults) {
    FILE* o = stderr;
    fprintf(o, "\n");
    fprintf(o, "Usage: centrolign [options] sequences.fasta\n");
    fprintf(o, "\n");
    fprintf(o, "Aligns the sequences of a FASTA file (- reads standard input) on an AMD Instinct GPU and writes the alignment to standard\n");
    fprintf(o, "output: a CIGAR for two sequences, a GFA graph otherwise.\n");
    fprintf(o, "\n");
    fprintf(o, "Options:\n");
    fprintf(o, " --tree / -T FILE            Newick guide tree over the FASTA's sequence names [the sequences in FASTA order]\n");
    fprintf(o, " --all-pairs / -A PREFIX     Write the induced alignment of every pair of sequences to files starting with PREFIX\n");
    fprintf(o, " --all-subprobs / -S PREFIX  Write the alignment of every subtree to files starting with PREFIX\n");
    fprintf(o, " --subalignments / -s FILE   Write the aligned paths of every subproblem to FILE (which must not exist yet)\n");
    fprintf(o, " --cyclize / -c              Merge long tandem duplications into cycles of the final graph\n");
    fprintf(o, " --cyclizing-size / -y INT   With -c, merge tandem duplications longer than INT bases [%s]\n", config_value(defaults, "min_cyclizing_length").c_str());
    fprintf(o, " --max-count / -m INT        Use an anchor only if it occurs at most INT times [%s]\n", config_value(defaults, "max_count").c_str());
    fprintf(o, " --max-anchors / -a INT      Consider at most INT anchors per merge [%s]\n", config_value(defaults, "max_num_match_pairs").c_str());
    fprintf(o, " --count-power / -p FLOAT    Divide anchor weights by the count raised to FLOAT [%s]\n", config_value(defaults, "pair_count_power").c_str());
    fprintf(o, " --chain-alg / -g INT        Chaining algorithm: 1 (sparse), 2 (sparse affine) [%s]\n", config_value(defaults, "chaining_algorithm").c_str());
    fprintf(o, " --no-unaln / -u             Do not look for unalignable regions\n");
    fprintf(o, " --verbosity / -v INT        0 (silent), 1 (minimal), 2 (basic), 3 (verbose), 4 (debug) [%s]\n", config_value(defaults, "logging_level").c_str());
    fprintf(o, " --config / -C FILE          Take every parameter from this config file (overrides all other command line input)\n");
    fprintf(o, " --generate-config / -G      Write a config file with the current parameters to standard output and exit\n");
    fprintf(o, " --restart / -R              Resume an interrupted run (the first run needs -S)\n");
    fprintf(o, " --threads / -t INT          Worker contexts that run calibrations and independent merges side by side [%s]\n", config_value(defaults, "threads").c_str());
    fprintf(o, " --skip-calibration          Keep the starting score scale instead of calibrating it to the input\n");
    fprintf(o, " --force-gfa-output          Write a GFA even for two sequences\n");
    fprintf(o, " --bond-prefix PREFIX        With -c, write the alignment of every tandem duplication found to files starting with PREFIX\n");
    fprintf(o, " --devices LIST              Comma-separated GPU ordinals the worker contexts are spread over [the first GPU]\n");
    fprintf(o, " --infer-tree                Infer the guide tree from k-mer distances (k = 21, neighbor joining) instead of taking one\n");
    fprintf(o, " --refine-tree INT           Rebuild the guide tree from the distances of an alignment made under it, up to INT times, then align\n");
    fprintf(o, " --tree-out FILE             With --infer-tree or --refine-tree, write the Newick tree the alignment used to FILE\n");
    fprintf(o, " --pair-stats FILE           Write matches, mismatches, gap bases, runs and distance of every pair of sequences to FILE (which must not exist yet)\n");
    fprintf(o, " --dist-out FILE             Write the matrix of pairwise alignment distances, in FASTA order, to FILE\n");
    fprintf(o, " --pair-profile FILE         Write matches, mismatches and gap bases of every pair of sequences per window of the first one to FILE (which must not exist yet; not with -c)\n");
    fprintf(o, " --window INT                With --pair-profile, the window in bases of the first sequence [1000]\n");
    fprintf(o, " --pair-events FILE          Write every insertion and deletion of at least --min-event bases between two sequences, with its positions, to FILE (which must not exist yet; not with -c)\n");
    fprintf(o, " --min-event INT             With --pair-events, the least length of an insertion or deletion that is written [50]\n");
    fprintf(o, " --compare-to GFA            With --pair-agreement, the baseline graph of the same sequences: an earlier run's, the reference's, a truth graph\n");
    fprintf(o, " --pair-agreement FILE       Write the aligned base pairs of every pair of sequences here, in the baseline and in both, to FILE (which must not exist yet; not with -c)\n");
    fprintf(o, " --graph GFA                 With --compare-to and --pair-agreement, compare GFA as the graph this run would have printed: nothing is aligned or printed\n");
    fprintf(o, " --msa-out FILE              Write the alignment as aligned FASTA, one row per sequence, to FILE (which must not exist yet; not with -c)\n");
    fprintf(o, " --column-stats FILE         Write the base and gap counts, the consensus and the site flag of every alignment column to FILE (which must not exist yet; not with -c)\n");
    fprintf(o, " --variable-sites FILE       Write the aligned FASTA of the variable sites alone, the site = 1 columns of --column-stats, to FILE (which must not exist yet; not with -c)\n");
    fprintf(o, " --msa-layout WORD           With the three above, the columns: level (compact, bubble branches side by side) or node (one graph node per column) [level]\n");
    fprintf(o, " --site-min-minor INT        A column is a variable site if its second most frequent base occurs at least INT times [1]\n");
    fprintf(o, " --site-max-gaps INT         ... and it has at most INT gaps [no limit]\n");
    fprintf(o, " --dotplot FILE              Write the windowed k-mer identity map (dot plot) of the input sequences, one row per kept window pair, to FILE (which must not exist yet)\n");
    fprintf(o, " --dotplot-k INT             With --dotplot, the k-mer length, 1 to 31 [21]\n");
    fprintf(o, " --dotplot-window INT        With --dotplot, the window in bases, k to 1048576 [2000]\n");
    fprintf(o, " --dotplot-min-identity FLOAT  With --dotplot, keep a window pair from this identity in percent on [86]\n");
    fprintf(o, " --dotplot-pairs all|self    With --dotplot, compare all windows or only the windows of the same sequence [all]\n");
    fprintf(o, " --dotplot-only              With --dotplot, end after writing the map: nothing is aligned or printed\n");
    fprintf(o, " --periods FILE              Write the repeat period spectra of the input sequences, one row per peak of every sequence and window, to FILE (which must not exist yet)\n");
    fprintf(o, " --periods-hist FILE         With --periods, write the non-zero bins of every spectrum to FILE (which must not exist yet)\n");
    fprintf(o, " --periods-k INT             With --periods, the k-mer length, 1 to 31 [8]\n");
    fprintf(o, " --periods-window INT        With --periods, the window in bases, 1 to 1048576 [10000]\n");
    fprintf(o, " --periods-max INT           With --periods, the longest period counted, 1 to 16383 [8000]\n");
    fprintf(o, " --periods-peaks INT         With --periods, the peaks written per row, 1 to 16 [3]\n");
    fprintf(o, " --periods-radius INT        With --periods, a peak is the largest count within INT bins on either side, 1 to 64 [1]\n");
    fprintf(o, " --periods-min-period INT    With --periods, the shortest period that can be a peak [1]\n");
    fprintf(o, " --periods-min-count INT     With --periods, the least count of a peak [2]\n");
    fprintf(o, " --periods-scope WORD        With --periods, the rows written: both, sequences or windows [both]\n");
    fprintf(o, " --periods-only              With --periods, end after writing the spectra: nothing is aligned or printed\n");
    fprintf(o, " --monomers FILE             Write which monomer of --monomers-templates stands where on every input sequence, one row per block, to FILE (which must not exist yet)\n");
    fprintf(o, " --monomers-templates FASTA  With --monomers (required), the monomer templates: 1 to 1024 bases each, at most 8192 in all (both strands counted)\n");
    fprintf(o, " --monomers-summary FILE     With --monomers, write blocks, bases and score per sequence, template and strand to FILE (which must not exist yet)\n");
    fprintf(o, " --monomers-strands WORD     With --monomers, the strands of the templates that are tried: forward or both [forward]\n");
    fprintf(o, " --monomers-match INT        With --monomers, the score of a match, 1 to 64 [1]\n");
    fprintf(o, " --monomers-mismatch INT     With --monomers, the score of a mismatch, -64 to -1 [-1]\n");
    fprintf(o, " --monomers-insertion INT    With --monomers, the score of a sequence base next to no template base, -64 to -1 [-1]\n");
    fprintf(o, " --monomers-deletion INT     With --monomers, the score of a template base next to no sequence base, -64 to -1 [-1]\n");
    fprintf(o, " --monomers-chunk INT        With --monomers, the bases of a sequence that are decomposed at once, 64 to 1048576, or 0 for all of them [4096]\n");
    fprintf(o, " --monomers-overlap INT      With --monomers, the bases a chunk reads beyond either end, 0 to 1048576; two template lengths or more [512]\n");
    fprintf(o, " --monomers-only             With --monomers, end after writing the decomposition: nothing is aligned or printed\n");
    fprintf(o, " --monomers-rounds INT       With --monomers, refine the templates in up to INT rounds (1 to 64) of decompose, align, vote before the decomposition is written\n");
    fprintf(o, " --monomers-write-templates FASTA  With --monomers-rounds or seeds, write the final templates to FASTA (which must not exist yet)\n");
    fprintf(o, " --monomers-pileup FILE      With --monomers, write the per-column base counts of the blocks under the final templates to FILE (which must not exist yet)\n");
    fprintf(o, " --monomers-least-share INT  With --monomers, the per mille of match * length a block's score must reach to be counted, 0 to 1000 [0]\n");
    fprintf(o, " --monomers-seed-period INT  With --monomers, cut the templates from the first sequence, INT bases each (1 to 1024), instead of --monomers-templates\n");
    fprintf(o, " --monomers-seed-count INT   With --monomers-seed-period, the number of templates cut [1]\n");
    fprintf(o, " --monomers-seed-start INT   With --monomers-seed-period, the base of the first sequence at which the first template begins [0]\n");
    fprintf(o, " --help / -h                 Print this message and exit\n");
    fprintf(o, "\n");
    fprintf(o, "Differences from the reference centrolign: every failure is 'error: ...' with exit status 1; -p takes a decimal number;\n");
    fprintf(o, "-t sets worker contexts; --devices, --infer-tree, --refine-tree, --tree-out, --pair-stats, --dist-out, --pair-profile, --window,\n");
    fprintf(o, "--pair-events, --min-event, --compare-to, --pair-agreement, --graph, --msa-out, --column-stats, --variable-sites, --msa-layout,\n");
    fprintf(o, "--site-min-minor, --site-max-gaps, --dotplot, --dotplot-k, --dotplot-window, --dotplot-min-identity, --dotplot-pairs, --dotplot-only,\n");
    fprintf(o, "--periods, --periods-hist, --periods-k, --periods-window, --periods-max, --periods-peaks, --periods-radius, --periods-min-period,\n");
    fprintf(o, "--periods-min-count, --periods-scope, --periods-only, --monomers, --monomers-templates, --monomers-summary, --monomers-strands,\n");
    fprintf(o, "--monomers-match, --monomers-mismatch, --monomers-insertion, --monomers-deletion, --monomers-chunk, --monomers-overlap,\n");
    fprintf(o, "--monomers-only, --monomers-rounds, --monomers-write-templates, --monomers-pileup, --monomers-least-share, --monomers-seed-period,\n");
    fprintf(o, "--monomers-seed-count and --monomers-seed-start are added; -v gates this tool's own progress lines. See README.md.\n");
}

struct Owned {
    cl_config* cfg = nullptr;
    cl_config* defaults = nullptr;
    cl_context* ctx = nullptr;
    ~Owned() {
        if (ctx) cl_context_destroy(ctx);
        cl_config_free(cfg);
        cl_config_free(defaults);
    }
};

int run(int argc, char** argv) {
    Owned own;
    own.cfg = cl_config_default();
    own.defaults = cl_config_default();
    if (!own.cfg || !own.defaults) return fail("out of memory");
    cl_config* cfg = own.cfg;

    std::string config_name;
    std::string tree_out, pair_stats, dist_out, refine_arg, pair_profile, pair_events, window_arg, min_event_arg, compare_to, pair_agreement, graph_name;
    std::string msa_out, column_stats, variable_sites, msa_layout_arg, site_min_minor_arg, site_max_gaps_arg;
    bool have_graph = false, have_msa_layout = false, have_site_min_minor = false, have_site_max_gaps = false;
    bool force_gfa_output = false, generate_config = false, infer_tree = false, have_window = false, have_min_event = false;
    std::string dotplot, dotplot_k_arg, dotplot_window_arg, dotplot_identity_arg, dotplot_pairs_arg;
    bool have_dotplot_k = false, have_dotplot_window = false, have_dotplot_identity = false, have_dotplot_pairs = false, dotplot_only = false;
    bool beside_dotplot_only = false;   // an option --dotplot-only does not go with
    std::string periods, periods_hist, periods_scope_arg;
    std::string periods_arg[7];   // --periods-k, -window, -max, -peaks, -radius, -min-period, -min-count as given
    bool have_periods_arg[7] = {false, false, false, false, false, false, false}, have_periods_scope = false, periods_only = false;
    bool beside_periods_only = false;   // an option --periods-only does not go with
    std::string monomers, monomers_templates, monomers_summary, monomers_strands_arg;
    std::string monomers_arg[6];   // --monomers-match, -mismatch, -insertion, -deletion, -chunk, -overlap as given
    bool have_monomers_arg[6] = {false, false, false, false, false, false}, have_monomers_strands = false, monomers_only = false;
    bool beside_monomers_only = false;   // an option --monomers-only does not go with
    std::string monomers_more[7];   // --monomers-rounds, -write-templates, -pileup, -least-share, -seed-period, -seed-count, -seed-start as given
    bool have_monomers_more[7] = {false, false, false, false, false, false, false};
    std::vector<int> devices;

    enum { OPT_SKIP_CALIBRATION = 1000, OPT_FORCE_GFA_OUTPUT = 1001, OPT_BOND_PREFIX = 1003, OPT_DEVICES = 1004, OPT_INFER_TREE = 1005, OPT_TREE_OUT = 1006,
           OPT_PAIR_STATS = 1007, OPT_DIST_OUT = 1008, OPT_REFINE_TREE = 1009,
           OPT_PAIR_PROFILE = 1010, OPT_WINDOW = 1011, OPT_PAIR_EVENTS = 1012, OPT_MIN_EVENT = 1013,
           OPT_COMPARE_TO = 1014, OPT_PAIR_AGREEMENT = 1015, OPT_GRAPH = 1016,
           OPT_MSA_OUT = 1017, OPT_COLUMN_STATS = 1018, OPT_VARIABLE_SITES = 1019, OPT_MSA_LAYOUT = 1020, OPT_SITE_MIN_MINOR = 1021, OPT_SITE_MAX_GAPS = 1022,
           OPT_DOTPLOT = 1023, OPT_DOTPLOT_K = 1024, OPT_DOTPLOT_WINDOW = 1025, OPT_DOTPLOT_MIN_IDENTITY = 1026, OPT_DOTPLOT_PAIRS = 1027, OPT_DOTPLOT_ONLY = 1028,
           OPT_PERIODS = 1029, OPT_PERIODS_HIST = 1030, OPT_PERIODS_K = 1031, OPT_PERIODS_WINDOW = 1032, OPT_PERIODS_MAX = 1033, OPT_PERIODS_PEAKS = 1034,
           OPT_PERIODS_RADIUS = 1035, OPT_PERIODS_MIN_PERIOD = 1036, OPT_PERIODS_MIN_COUNT = 1037, OPT_PERIODS_SCOPE = 1038, OPT_PERIODS_ONLY = 1039,
           OPT_MONOMERS = 1040, OPT_MONOMERS_TEMPLATES = 1041, OPT_MONOMERS_SUMMARY = 1042, OPT_MONOMERS_STRANDS = 1043, OPT_MONOMERS_MATCH = 1044,
           OPT_MONOMERS_MISMATCH = 1045, OPT_MONOMERS_INSERTION = 1046, OPT_MONOMERS_DELETION = 1047, OPT_MONOMERS_CHUNK = 1048, OPT_MONOMERS_OVERLAP = 1049,
           OPT_MONOMERS_ONLY = 1050, OPT_MONOMERS_ROUNDS = 1051, OPT_MONOMERS_WRITE_TEMPLATES = 1052, OPT_MONOMERS_PILEUP = 1053, OPT_MONOMERS_LEAST_SHARE = 1054,
           OPT_MONOMERS_SEED_PERIOD = 1055, OPT_MONOMERS_SEED_COUNT = 1056, OPT_MONOMERS_SEED_START = 1057 };
    static const struct option options[] = {
        {"tree", required_argument, nullptr, 'T'},
        {"all-pairs", required_argument, nullptr, 'A'},
        {"all-subprobs", required_argument, nullptr, 'S'},
        {"subalignments", required_argument, nullptr, 's'},
        {"cyclize", no_argument, nullptr, 'c'},
        {"cyclizing-size", required_argument, nullptr, 'y'},
        {"max-count", required_argument, nullptr, 'm'},
        {"max-anchors", required_argument, nullptr, 'a'},
        {"count-power", required_argument, nullptr, 'p'},
        {"chain-alg", required_argument, nullptr, 'g'},
        {"no-unaln", no_argument, nullptr, 'u'},
        {"verbosity", required_argument, nullptr, 'v'},
        {"config", required_argument, nullptr, 'C'},
        {"generate-config", no_argument, nullptr, 'G'},
        {"restart", no_argument, nullptr, 'R'},
        {"threads", required_argument, nullptr, 't'},
        {"help", no_argument, nullptr, 'h'},
        {"skip-calibration", no_argument, nullptr, OPT_SKIP_CALIBRATION},
        {"force-gfa-output", no_argument, nullptr, OPT_FORCE_GFA_OUTPUT},
        {"bond-prefix", required_argument, nullptr, OPT_BOND_PREFIX},
        {"devices", required_argument, nullptr, OPT_DEVICES},
        {"infer-tree", no_argument, nullptr, OPT_INFER_TREE},
        {"tree-out", required_argument, nullptr, OPT_TREE_OUT},
        {"pair-stats", required_argument, nullptr, OPT_PAIR_STATS},
        {"dist-out", required_argument, nullptr, OPT_DIST_OUT},
        {"refine-tree", required_argument, nullptr, OPT_REFINE_TREE},
        {"pair-profile", required_argument, nullptr, OPT_PAIR_PROFILE},
        {"window", required_argument, nullptr, OPT_WINDOW},
        {"pair-events", required_argument, nullptr, OPT_PAIR_EVENTS},
        {"min-event", required_argument, nullptr, OPT_MIN_EVENT},
        {"compare-to", required_argument, nullptr, OPT_COMPARE_TO},
        {"pair-agreement", required_argument, nullptr, OPT_PAIR_AGREEMENT},
        {"graph", required_argument, nullptr, OPT_GRAPH},
        {"msa-out", required_argument, nullptr, OPT_MSA_OUT},
        {"column-stats", required_argument, nullptr, OPT_COLUMN_STATS},
        {"variable-sites", required_argument, nullptr, OPT_VARIABLE_SITES},
        {"msa-layout", required_argument, nullptr, OPT_MSA_LAYOUT},
        {"site-min-minor", required_argument, nullptr, OPT_SITE_MIN_MINOR},
        {"site-max-gaps", required_argument, nullptr, OPT_SITE_MAX_GAPS},
        {"dotplot", required_argument, nullptr, OPT_DOTPLOT},
        {"dotplot-k", required_argument, nullptr, OPT_DOTPLOT_K},
        {"dotplot-window", required_argument, nullptr, OPT_DOTPLOT_WINDOW},
        {"dotplot-min-identity", required_argument, nullptr, OPT_DOTPLOT_MIN_IDENTITY},
        {"dotplot-pairs", required_argument, nullptr, OPT_DOTPLOT_PAIRS},
        {"dotplot-only", no_argument, nullptr, OPT_DOTPLOT_ONLY},
        {"periods", required_argument, nullptr, OPT_PERIODS},
        {"periods-hist", required_argument, nullptr, OPT_PERIODS_HIST},
        {"periods-k", required_argument, nullptr, OPT_PERIODS_K},
        {"periods-window", required_argument, nullptr, OPT_PERIODS_WINDOW},
        {"periods-max", required_argument, nullptr, OPT_PERIODS_MAX},
        {"periods-peaks", required_argument, nullptr, OPT_PERIODS_PEAKS},
        {"periods-radius", required_argument, nullptr, OPT_PERIODS_RADIUS},
        {"periods-min-period", required_argument, nullptr, OPT_PERIODS_MIN_PERIOD},
        {"periods-min-count", required_argument, nullptr, OPT_PERIODS_MIN_COUNT},
        {"periods-scope", required_argument, nullptr, OPT_PERIODS_SCOPE},
        {"periods-only", no_argument, nullptr, OPT_PERIODS_ONLY},
        {"monomers", required_argument, nullptr, OPT_MONOMERS},
        {"monomers-templates", required_argument, nullptr, OPT_MONOMERS_TEMPLATES},
        {"monomers-summary", required_argument, nullptr, OPT_MONOMERS_SUMMARY},
        {"monomers-strands", required_argument, nullptr, OPT_MONOMERS_STRANDS},
        {"monomers-match", required_argument, nullptr, OPT_MONOMERS_MATCH},
        {"monomers-mismatch", required_argument, nullptr, OPT_MONOMERS_MISMATCH},
        {"monomers-insertion", required_argument, nullptr, OPT_MONOMERS_INSERTION},
        {"monomers-deletion", required_argument, nullptr, OPT_MONOMERS_DELETION},
        {"monomers-chunk", required_argument, nullptr, OPT_MONOMERS_CHUNK},
        {"monomers-overlap", required_argument, nullptr, OPT_MONOMERS_OVERLAP},
        {"monomers-only", no_argument, nullptr, OPT_MONOMERS_ONLY},
        {"monomers-rounds", required_argument, nullptr, OPT_MONOMERS_ROUNDS},
        {"monomers-write-templates", required_argument, nullptr, OPT_MONOMERS_WRITE_TEMPLATES},
        {"monomers-pileup", required_argument, nullptr, OPT_MONOMERS_PILEUP},
        {"monomers-least-share", required_argument, nullptr, OPT_MONOMERS_LEAST_SHARE},
        {"monomers-seed-period", required_argument, nullptr, OPT_MONOMERS_SEED_PERIOD},
        {"monomers-seed-count", required_argument, nullptr, OPT_MONOMERS_SEED_COUNT},
        {"monomers-seed-start", required_argument, nullptr, OPT_MONOMERS_SEED_START},
        {nullptr, 0, nullptr, 0},
    };
    opterr = 0;   // reported here, as "error: ..."
    while (true) {
        const int o = getopt_long(argc, argv, ":T:A:S:s:cy:m:a:p:g:uv:C:GRt:h", options, nullptr);
        if (o == -1) break;
        const char* name = nullptr;   // the parameter this option sets from its argument
        const char* value = optarg;
        if (o != 'v' && o != OPT_DEVICES && !(o >= OPT_DOTPLOT && o <= OPT_DOTPLOT_ONLY)) beside_dotplot_only = true;
        if (o != 'v' && o != OPT_DEVICES && !(o >= OPT_PERIODS && o <= OPT_PERIODS_ONLY)) beside_periods_only = true;
        if (o != 'v' && o != OPT_DEVICES && !(o >= OPT_MONOMERS && o <= OPT_MONOMERS_SEED_START)) beside_monomers_only = true;
        switch (o) {
        case 'T': name = "tree_name"; break;
        case 'A': name = "all_pairs_prefix"; break;
        case 'S': name = "subproblems_prefix"; break;
        case 's': name = "subalignments_filepath"; break;
        case 'c': name = "cyclize_tandem_duplications"; value = "true"; break;
        case 'y': name = "min_cyclizing_length"; break;
        case 'm': name = "max_count"; break;
        case 'a': name = "max_num_match_pairs"; break;
        case 'p': name = "pair_count_power"; break;
        case 'g': name = "chaining_algorithm"; break;
        case 'u': name = "constraint_method"; value = "0"; break;
        case 'v': name = "logging_level"; break;
        case 'C': config_name = optarg; break;
        case 'G': generate_config = true; break;
        case 'R': name = "restart"; value = "true"; break;
        case 't': name = "threads"; break;
        case 'h': print_help(own.defaults); return 0;
        case OPT_SKIP_CALIBRATION: name = "skip_calibration"; value = "true"; break;
        case OPT_FORCE_GFA_OUTPUT: force_gfa_output = true; break;
        case OPT_BOND_PREFIX: name = "bonds_prefix"; break;
        case OPT_DEVICES:
            if (!parse_devices(optarg, devices)) return fail(std::string("--devices expects comma-separated device ordinals, got '") + optarg + "'");
            break;
        case OPT_INFER_TREE: infer_tree = true; break;
        case OPT_TREE_OUT: tree_out = optarg; break;
        case OPT_PAIR_STATS: pair_stats = optarg; break;
        case OPT_DIST_OUT: dist_out = optarg; break;
        case OPT_REFINE_TREE: refine_arg = optarg; break;
        case OPT_PAIR_PROFILE: pair_profile = optarg; break;
        case OPT_WINDOW: window_arg = optarg; have_window = true; break;
        case OPT_PAIR_EVENTS: pair_events = optarg; break;
        case OPT_MIN_EVENT: min_event_arg = optarg; have_min_event = true; break;
        case OPT_COMPARE_TO: compare_to = optarg; break;
        case OPT_PAIR_AGREEMENT: pair_agreement = optarg; break;
        case OPT_GRAPH: graph_name = optarg; have_graph = true; break;
        case OPT_MSA_OUT: msa_out = optarg; break;
        case OPT_COLUMN_STATS: column_stats = optarg; break;
        case OPT_VARIABLE_SITES: variable_sites = optarg; break;
        case OPT_MSA_LAYOUT: msa_layout_arg = optarg; have_msa_layout = true; break;
        case OPT_SITE_MIN_MINOR: site_min_minor_arg = optarg; have_site_min_minor = true; break;
        case OPT_SITE_MAX_GAPS: site_max_gaps_arg = optarg; have_site_max_gaps = true; break;
        case OPT_DOTPLOT: dotplot = optarg; break;
        case OPT_DOTPLOT_K: dotplot_k_arg = optarg; have_dotplot_k = true; break;
        case OPT_DOTPLOT_WINDOW: dotplot_window_arg = optarg; have_dotplot_window = true; break;
        case OPT_DOTPLOT_MIN_IDENTITY: dotplot_identity_arg = optarg; have_dotplot_identity = true; break;
        case OPT_DOTPLOT_PAIRS: dotplot_pairs_arg = optarg; have_dotplot_pairs = true; break;
        case OPT_DOTPLOT_ONLY: dotplot_only = true; break;
        case OPT_PERIODS: periods = optarg; break;
        case OPT_PERIODS_HIST: periods_hist = optarg; break;
        case OPT_PERIODS_K: case OPT_PERIODS_WINDOW: case OPT_PERIODS_MAX: case OPT_PERIODS_PEAKS: case OPT_PERIODS_RADIUS: case OPT_PERIODS_MIN_PERIOD:
        case OPT_PERIODS_MIN_COUNT:
            periods_arg[o - OPT_PERIODS_K] = optarg;
            have_periods_arg[o - OPT_PERIODS_K] = true;
            break;
        case OPT_PERIODS_SCOPE: periods_scope_arg = optarg; have_periods_scope = true; break;
        case OPT_PERIODS_ONLY: periods_only = true; break;
        case OPT_MONOMERS: monomers = optarg; break;
        case OPT_MONOMERS_TEMPLATES: monomers_templates = optarg; break;
        case OPT_MONOMERS_SUMMARY: monomers_summary = optarg; break;
        case OPT_MONOMERS_STRANDS: monomers_strands_arg = optarg; have_monomers_strands = true; break;
        case OPT_MONOMERS_MATCH: case OPT_MONOMERS_MISMATCH: case OPT_MONOMERS_INSERTION: case OPT_MONOMERS_DELETION: case OPT_MONOMERS_CHUNK:
        case OPT_MONOMERS_OVERLAP:
            monomers_arg[o - OPT_MONOMERS_MATCH] = optarg;
            have_monomers_arg[o - OPT_MONOMERS_MATCH] = true;
            break;
        case OPT_MONOMERS_ONLY: monomers_only = true; break;
        case OPT_MONOMERS_ROUNDS: case OPT_MONOMERS_WRITE_TEMPLATES: case OPT_MONOMERS_PILEUP: case OPT_MONOMERS_LEAST_SHARE: case OPT_MONOMERS_SEED_PERIOD:
        case OPT_MONOMERS_SEED_COUNT: case OPT_MONOMERS_SEED_START:
            monomers_more[o - OPT_MONOMERS_ROUNDS] = optarg;
            have_monomers_more[o - OPT_MONOMERS_ROUNDS] = true;
            break;
        case ':':
        default: {
            // optopt names a short option; a long one is the argument getopt just stepped over
            const std::string opt = optopt > 0 && optopt < 128 ? std::string("-") + (char)optopt : std::string(optind > 0 && optind <= argc ? argv[optind - 1] : "");
            fprintf(stderr, o == ':' ? "error: option '%s' requires an argument\n" : "error: unknown option '%s'\n", opt.c_str());
            print_help(own.defaults);
            return 1;
        }
        }
        if (name && cl_config_set(cfg, name, value)) return fail(lib_error());
    }

    const int n_positional = argc - optind;
    if (n_positional > 1) {
        fprintf(stderr, "error: expected between 0 and 1 positional arguments but got %d\n", n_positional);
        print_help(own.defaults);
        return 1;
    }
    if (n_positional == 1 && cl_config_set(cfg, "fasta_name", argv[optind])) return fail(lib_error());

    if (generate_config) {
        const std::string text = generate(cfg);
        fwrite(text.data(), 1, text.size(), stdout);
        return fflush(stdout) == 0 ? 0 : fail("could not write the config to standard output");
    }

    // --graph stands in for the whole run: it goes with the two comparison options and with nothing that reads an input or writes another output
    if (have_graph) {
        if (compare_to.empty() || pair_agreement.empty()) return fail("--graph needs --compare-to and --pair-agreement");
        if (n_positional == 1) return fail("--graph cannot be combined with a FASTA: it takes the place of the alignment");
        if (!config_value(cfg, "tree_name").empty() || infer_tree || !refine_arg.empty()) return fail("--graph cannot be combined with a guide tree (-T, --infer-tree, --refine-tree)");
        if (!config_name.empty()) return fail("--graph cannot be combined with a config file (-C)");
        if (config_value(cfg, "restart") == "true") return fail("--graph cannot be combined with a restart (-R)");
        for (const char* name : {"all_pairs_prefix", "subproblems_prefix", "subalignments_filepath", "bonds_prefix"})
            if (!config_value(cfg, name).empty()) return fail("--graph cannot be combined with another output option (-A, -S, -s, --bond-prefix)");
        if (!tree_out.empty() || !pair_stats.empty() || !dist_out.empty() || !pair_profile.empty() || !pair_events.empty() || have_window || have_min_event)
            return fail("--graph cannot be combined with another output option (--tree-out, --pair-stats, --dist-out, --pair-profile, --pair-events)");
        if (!msa_out.empty() || !column_stats.empty() || !variable_sites.empty() || have_msa_layout || have_site_min_minor || have_site_max_gaps)
            return fail("--graph cannot be combined with another output option (--msa-out, --column-stats, --variable-sites)");
    }

    if (dotplot_only && !dotplot.empty() && beside_dotplot_only)
        return fail("--dotplot-only goes with the --dotplot options, -v and --devices alone: nothing else is run");
    if (periods_only && !periods.empty() && beside_periods_only)
        return fail("--periods-only goes with the --periods options, -v and --devices alone: nothing else is run");
    if (monomers_only && !monomers.empty() && beside_monomers_only)
        return fail("--monomers-only goes with the --monomers options, -v and --devices alone: nothing else is run");
    if (!config_name.empty()) {
        if (generate(cfg) != generate(own.defaults))
            fprintf(stderr, "warning: All other command-line arguments are being overridden by config file parameters.\n\n");
        std::string text, err;
        if (!read_input(config_name, text, err)) return fail(err);
        cl_config* parsed = nullptr;
        if (cl_config_parse(text.data(), text.size(), &parsed)) return fail(lib_error());
        cl_config_free(own.cfg);
        cfg = own.cfg = parsed;
    }

    // --dotplot and its options, checked before anything is read or opened
    cl_dotplot_params dotplot_params;
    cl_dotplot_params_default(&dotplot_params);
    if (dotplot.empty()) {
        const char* lone = have_dotplot_k ? "--dotplot-k" : have_dotplot_window ? "--dotplot-window" : have_dotplot_identity ? "--dotplot-min-identity"
                           : have_dotplot_pairs ? "--dotplot-pairs" : dotplot_only ? "--dotplot-only" : nullptr;
        if (lone) return fail(std::string(lone) + " needs --dotplot");
    } else {
        if (have_graph) return fail("--dotplot cannot be combined with --graph: it reads the sequences of a FASTA");
        uint64_t v = 0;
        if (have_dotplot_k && (!parse_positive(dotplot_k_arg, v) || v > 31)) return fail("--dotplot-k expects a k-mer length from 1 to 31, got '" + dotplot_k_arg + "'");
        if (have_dotplot_k) dotplot_params.k = (int)v;
        if (have_dotplot_window && (!parse_positive(dotplot_window_arg, v) || v > (1u << 20) || v < (uint64_t)dotplot_params.k))
            return fail("--dotplot-window expects a whole number of bases from k = " + std::to_string(dotplot_params.k) + " to 1048576, got '" + dotplot_window_arg + "'");
        if (have_dotplot_window) dotplot_params.window = (uint32_t)v;
        if (dotplot_params.window < (uint32_t)dotplot_params.k) return fail("--dotplot-k " + dotplot_k_arg + " is more than the window of " + std::to_string(dotplot_params.window) + " bases");
        if (have_dotplot_identity) {
            char* end = nullptr;
            errno = 0;
            const double x = strtod(dotplot_identity_arg.c_str(), &end);
            if (dotplot_identity_arg.empty() || *end || errno || !(x >= 0.0 && x <= 100.0))
                return fail("--dotplot-min-identity expects a percentage from 0 to 100, got '" + dotplot_identity_arg + "'");
            dotplot_params.min_identity = x;
        }
        if (have_dotplot_pairs) {
            if (dotplot_pairs_arg == "all") dotplot_params.pairs = 0;
            else if (dotplot_pairs_arg == "self") dotplot_params.pairs = 1;
            else return fail("--dotplot-pairs expects all or self, got '" + dotplot_pairs_arg + "'");
        }
        if (std::ifstream(dotplot).good()) return fail("Dot plot file already exists: " + dotplot);
        const std::string others[10] = {tree_out, pair_stats, dist_out, pair_profile, pair_events, pair_agreement, msa_out, column_stats, variable_sites,
                                        config_value(cfg, "subalignments_filepath")};
        for (const std::string& other : others)
            if (dotplot == other) return fail("--dotplot names the file of another output option");
    }
    // --periods and its options, checked the same way
    cl_periods_params periods_params;
    cl_periods_params_default(&periods_params);
    int periods_scope = 0;
    {
        struct { const char* opt; const char* what; uint64_t most; } const numbers[7] = {
            {"--periods-k", "a k-mer length from 1 to 31", 31}, {"--periods-window", "a whole number of bases from 1 to 1048576", 1u << 20},
            {"--periods-max", "a period from 1 to 16383", 16383}, {"--periods-peaks", "a number of peaks from 1 to 16", 16},
            {"--periods-radius", "a number of bins from 1 to 64", 64}, {"--periods-min-period", "a period, at least 1", 0xFFFFFFFFull},
            {"--periods-min-count", "a count, at least 1", 0xFFFFFFFFull}};
        if (periods.empty()) {
            const char* lone = !periods_hist.empty() ? "--periods-hist" : have_periods_scope ? "--periods-scope" : periods_only ? "--periods-only" : nullptr;
            for (int i = 6; i >= 0; --i) if (have_periods_arg[i]) lone = numbers[i].opt;
            if (lone) return fail(std::string(lone) + " needs --periods");
        } else {
            if (have_graph) return fail("--periods cannot be combined with --graph: it reads the sequences of a FASTA");
            uint64_t v[7] = {0, 0, 0, 0, 0, 0, 0};
            for (int i = 0; i < 7; ++i)
                if (have_periods_arg[i] && (!parse_positive(periods_arg[i], v[i]) || v[i] > numbers[i].most))
                    return fail(std::string(numbers[i].opt) + " expects " + numbers[i].what + ", got '" + periods_arg[i] + "'");
            if (have_periods_arg[0]) periods_params.k = (int)v[0];
            uint32_t* const into[7] = {nullptr, &periods_params.window, &periods_params.max_period, &periods_params.n_peaks, &periods_params.peak_radius,
                                       &periods_params.min_period, &periods_params.min_count};
            for (int i = 1; i < 7; ++i) if (have_periods_arg[i]) *into[i] = (uint32_t)v[i];
            if (have_periods_scope) {
                if (periods_scope_arg == "both") periods_scope = 0;
                else if (periods_scope_arg == "sequences") periods_scope = 1;
                else if (periods_scope_arg == "windows") periods_scope = 2;
                else return fail("--periods-scope expects both, sequences or windows, got '" + periods_scope_arg + "'");
            }
            periods_params.want_hist = periods_hist.empty() ? 0 : 1;
            if (std::ifstream(periods).good()) return fail("Period spectra file already exists: " + periods);
            if (!periods_hist.empty() && std::ifstream(periods_hist).good()) return fail("Period histogram file already exists: " + periods_hist);
            if (periods == periods_hist) return fail("--periods and --periods-hist name the same file");
            const std::string others[11] = {tree_out, pair_stats, dist_out, pair_profile, pair_events, pair_agreement, msa_out, column_stats, variable_sites,
                                            config_value(cfg, "subalignments_filepath"), dotplot};
            for (const std::string& other : others)
                if (periods == other || (!periods_hist.empty() && periods_hist == other)) return fail("--periods and --periods-hist cannot name the file of another output option");
        }
    }
    // --monomers and its options, checked the same way; the templates are read here: what is wrong with them needs no other input
    cl_monomers_params monomers_params;
    cl_monomers_params_default(&monomers_params);
    MonomerTemplates monomer_templates;
    MonomerRefinement monomer_refinement;
    uint64_t monomer_seed[3] = {0, 1, 0};   // period (0: no seeds), count, start
    {
        static const char* const opts[6] = {"--monomers-match", "--monomers-mismatch", "--monomers-insertion", "--monomers-deletion", "--monomers-chunk", "--monomers-overlap"};
        static const char* const more_opts[7] = {"--monomers-rounds", "--monomers-write-templates", "--monomers-pileup", "--monomers-least-share", "--monomers-seed-period",
                                                 "--monomers-seed-count", "--monomers-seed-start"};
        if (monomers.empty()) {
            const char* lone = !monomers_templates.empty() ? "--monomers-templates" : !monomers_summary.empty() ? "--monomers-summary"
                               : have_monomers_strands ? "--monomers-strands" : monomers_only ? "--monomers-only" : nullptr;
            for (int i = 5; i >= 0; --i) if (have_monomers_arg[i]) lone = opts[i];
            for (int i = 6; i >= 0; --i) if (have_monomers_more[i]) lone = more_opts[i];
            if (lone) return fail(std::string(lone) + " needs --monomers");
        } else {
            if (have_graph) return fail("--monomers cannot be combined with --graph: it reads the sequences of a FASTA");
            if (monomers_templates.empty() && !have_monomers_more[4]) return fail("--monomers needs --monomers-templates or --monomers-seed-period");
            if (!monomers_templates.empty() && have_monomers_more[4]) return fail("--monomers-templates and --monomers-seed-period cannot both be given");
            if (!have_monomers_more[4] && (have_monomers_more[5] || have_monomers_more[6]))
                return fail(std::string(have_monomers_more[5] ? more_opts[5] : more_opts[6]) + " needs --monomers-seed-period");
            if (have_monomers_more[1] && !have_monomers_more[0] && !have_monomers_more[4])
                return fail("--monomers-write-templates needs --monomers-rounds or --monomers-seed-period: the given templates would be written back");
            uint64_t v = 0;
            if (have_monomers_arg[0] && (!parse_positive(monomers_arg[0], v) || v > 64)) return fail("--monomers-match expects a score from 1 to 64, got '" + monomers_arg[0] + "'");
            if (have_monomers_arg[0]) monomers_params.match = (int32_t)v;
            int32_t* const penalty[3] = {&monomers_params.mismatch, &monomers_params.insertion, &monomers_params.deletion};
            for (int i = 1; i <= 3; ++i) {
                if (!have_monomers_arg[i]) continue;
                char* end = nullptr;
                errno = 0;
                const long x = strtol(monomers_arg[i].c_str(), &end, 10);
                if (monomers_arg[i].empty() || *end || errno || x < -64 || x > -1) return fail(std::string(opts[i]) + " expects a score from -64 to -1, got '" + monomers_arg[i] + "'");
                *penalty[i - 1] = (int32_t)x;
            }
            if (have_monomers_arg[4] && (!parse_count(monomers_arg[4], v) || (v != 0 && v < 64) || v > (1u << 20)))
                return fail("--monomers-chunk expects 0 or a whole number of bases from 64 to 1048576, got '" + monomers_arg[4] + "'");
            if (have_monomers_arg[4]) monomers_params.chunk = (uint32_t)v;
            if (have_monomers_arg[5] && (!parse_count(monomers_arg[5], v) || v > (1u << 20)))
                return fail("--monomers-overlap expects a whole number of bases from 0 to 1048576, got '" + monomers_arg[5] + "'");
            if (have_monomers_arg[5]) monomers_params.overlap = (uint32_t)v;
            if (have_monomers_strands) {
                if (monomers_strands_arg == "forward") monomers_params.strands = 1;
                else if (monomers_strands_arg == "both") monomers_params.strands = 2;
                else return fail("--monomers-strands expects forward or both, got '" + monomers_strands_arg + "'");
            }
            if (std::ifstream(monomers).good()) return fail("Monomer decomposition file already exists: " + monomers);
            if (!monomers_summary.empty() && std::ifstream(monomers_summary).good()) return fail("Monomer summary file already exists: " + monomers_summary);
            if (monomers == monomers_summary) return fail("--monomers and --monomers-summary name the same file");
            const std::string others[13] = {tree_out, pair_stats, dist_out, pair_profile, pair_events, pair_agreement, msa_out, column_stats, variable_sites,
                                            config_value(cfg, "subalignments_filepath"), dotplot, periods, periods_hist};
            for (const std::string& other : others)
                if (!other.empty() && (monomers == other || monomers_summary == other))
                    return fail("--monomers and --monomers-summary cannot name the file of another output option");
            if (!monomers_templates.empty() && (monomers == monomers_templates || monomers_summary == monomers_templates))
                return fail("--monomers and --monomers-summary cannot name the templates' file");
            if (have_monomers_more[0]) {
                if (!parse_positive(monomers_more[0], v) || v > 64) return fail("--monomers-rounds expects a whole number of rounds from 1 to 64, got '" + monomers_more[0] + "'");
                monomer_refinement.rounds = (uint32_t)v;
            }
            if (have_monomers_more[3]) {
                if (!parse_count(monomers_more[3], v) || v > 1000) return fail("--monomers-least-share expects a whole number of per mille from 0 to 1000, got '" + monomers_more[3] + "'");
                monomer_refinement.least_share = (uint32_t)v;
            }
            if (have_monomers_more[4]) {
                if (!parse_positive(monomers_more[4], v) || v > 1024) return fail("--monomers-seed-period expects a whole number of bases from 1 to 1024, got '" + monomers_more[4] + "'");
                monomer_seed[0] = v;
                if (have_monomers_more[5] && (!parse_positive(monomers_more[5], v) || v > 8192))
                    return fail("--monomers-seed-count expects a whole number of templates from 1 on, got '" + monomers_more[5] + "'");
                if (have_monomers_more[5]) monomer_seed[1] = v;
                if (monomer_seed[0] * monomer_seed[1] * (uint64_t)monomers_params.strands > 8192)
                    return fail("--monomers-seed-count: " + std::to_string(monomer_seed[1]) + " templates of " + std::to_string(monomer_seed[0]) +
                                " bases are more than 8192 template bases in all (both strands counted)");
                if (have_monomers_more[6] && (!parse_count(monomers_more[6], v) || v >= (1ull << 30)))
                    return fail("--monomers-seed-start expects a whole number of bases below 2^30, got '" + monomers_more[6] + "'");
                if (have_monomers_more[6]) monomer_seed[2] = v;
            }
            monomer_refinement.templates_file = monomers_more[1];
            monomer_refinement.pileup_file = monomers_more[2];
            for (int i = 1; i <= 2; ++i) {
                const std::string& made = monomers_more[i];
                if (!have_monomers_more[i]) continue;
                if (made.empty()) return fail(std::string(more_opts[i]) + " expects a file name");
                if (std::ifstream(made).good()) return fail(std::string(i == 1 ? "Monomer templates" : "Monomer pileup") + " file already exists: " + made);
                if (made == monomers || made == monomers_summary || made == monomers_templates || (i == 2 && made == monomers_more[1]))
                    return fail(std::string(more_opts[i]) + " cannot name the file of another --monomers option");
                for (const std::string& other : others)
                    if (made == other) return fail(std::string(more_opts[i]) + " cannot name the file of another output option");
            }
            std::string err;
            if (!monomers_templates.empty() && !read_monomer_templates(monomers_templates, monomers_params.strands, monomer_templates, err)) return fail(err);
        }
    }
    // the tree options of this project, checked before anything is read or opened
    if (infer_tree && !config_value(cfg, "tree_name").empty()) return fail("--infer-tree cannot be combined with a guide tree (-T or tree_name)");
    if (!tree_out.empty() && !infer_tree && refine_arg.empty()) return fail("--tree-out needs --infer-tree");
    int refine_rounds = 0;
    if (!refine_arg.empty()) {
        char* end = nullptr;
        errno = 0;
        const long v = strtol(refine_arg.c_str(), &end, 10);
        if (*end || errno || v < 1 || v > 1000000) return fail("--refine-tree expects a whole number of rounds, at least 1, got '" + refine_arg + "'");
        refine_rounds = (int)v;
        if (config_value(cfg, "restart") == "true") return fail("--refine-tree cannot be combined with a restart (-R)");
    }
    if (!pair_stats.empty() && std::ifstream(pair_stats).good()) return fail("Pair statistics file already exists: " + pair_stats);
    // --pair-profile / --pair-events, also checked before anything is read or opened
    uint64_t window = 1000, min_event = 50;
    if (have_window && pair_profile.empty()) return fail("--window needs --pair-profile");
    if (have_min_event && pair_events.empty()) return fail("--min-event needs --pair-events");
    if (have_window && !parse_positive(window_arg, window)) return fail("--window expects a whole number of bases, at least 1, got '" + window_arg + "'");
    if (have_min_event && !parse_positive(min_event_arg, min_event))
        return fail("--min-event expects a whole number of bases, at least 1, got '" + min_event_arg + "'");
    if (!pair_profile.empty() && std::ifstream(pair_profile).good()) return fail("Pair profile file already exists: " + pair_profile);
    if (!pair_events.empty() && std::ifstream(pair_events).good()) return fail("Pair events file already exists: " + pair_events);
    if (!pair_profile.empty() && pair_profile == pair_events) return fail("--pair-profile and --pair-events name the same file");
    const bool pair_positions = !pair_profile.empty() || !pair_events.empty();
    if (pair_positions && config_value(cfg, "cyclize_tandem_duplications") == "true")
        return fail("--pair-profile and --pair-events cannot be combined with -c: the final graph then has cycles");
    // --compare-to / --pair-agreement, checked the same way; the baseline is read here: what is wrong with it needs no other input
    if (compare_to.empty() != pair_agreement.empty()) return fail(compare_to.empty() ? "--pair-agreement needs --compare-to" : "--compare-to needs --pair-agreement");
    const bool agreement = !pair_agreement.empty();
    if (agreement && std::ifstream(pair_agreement).good()) return fail("Pair agreement file already exists: " + pair_agreement);
    if (agreement && (pair_agreement == pair_profile || pair_agreement == pair_events || pair_agreement == pair_stats || pair_agreement == dist_out))
        return fail("--pair-agreement names the file of another output option");
    if (agreement && config_value(cfg, "cyclize_tandem_duplications") == "true")
        return fail("--compare-to and --pair-agreement cannot be combined with -c: the final graph then has cycles");
    // --msa-out / --column-stats / --variable-sites, checked the same way
    const bool msa_columns = !msa_out.empty() || !column_stats.empty() || !variable_sites.empty();
    const bool msa_sites = !column_stats.empty() || !variable_sites.empty();
    int msa_layout = 0;
    uint64_t site_min_minor = 1, site_max_gaps = 0xFFFFFFFFull;
    if (have_msa_layout && !msa_columns) return fail("--msa-layout needs --msa-out, --column-stats or --variable-sites");
    if ((have_site_min_minor || have_site_max_gaps) && !msa_sites)
        return fail(std::string(have_site_min_minor ? "--site-min-minor" : "--site-max-gaps") + " needs --column-stats or --variable-sites");
    if (have_msa_layout) {
        if (msa_layout_arg == "level") msa_layout = 0;
        else if (msa_layout_arg == "node") msa_layout = 1;
        else return fail("--msa-layout expects level or node, got '" + msa_layout_arg + "'");
    }
    if (have_site_min_minor && !parse_positive(site_min_minor_arg, site_min_minor))
        return fail("--site-min-minor expects a whole number of sequences, at least 1, got '" + site_min_minor_arg + "'");
    if (have_site_max_gaps && !parse_count(site_max_gaps_arg, site_max_gaps))
        return fail("--site-max-gaps expects a whole number of sequences, at least 0, got '" + site_max_gaps_arg + "'");
    site_min_minor = std::min<uint64_t>(site_min_minor, 0xFFFFFFFFull);   // (more than any number of sequences either way)
    site_max_gaps = std::min<uint64_t>(site_max_gaps, 0xFFFFFFFFull);
    if (!msa_out.empty() && std::ifstream(msa_out).good()) return fail("MSA file already exists: " + msa_out);
    if (!column_stats.empty() && std::ifstream(column_stats).good()) return fail("Column statistics file already exists: " + column_stats);
    if (!variable_sites.empty() && std::ifstream(variable_sites).good()) return fail("Variable sites file already exists: " + variable_sites);
    if (msa_columns) {
        const std::string* mine[3] = {&msa_out, &column_stats, &variable_sites};
        const std::string others[7] = {pair_stats, dist_out, pair_profile, pair_events, pair_agreement, tree_out, config_value(cfg, "subalignments_filepath")};
        for (int a = 0; a < 3; ++a) {
            if (mine[a]->empty()) continue;
            for (int b = a + 1; b < 3; ++b) if (*mine[a] == *mine[b]) return fail("--msa-out, --column-stats and --variable-sites must name different files");
            for (const std::string& other : others)
                if (*mine[a] == other) return fail("--msa-out, --column-stats and --variable-sites cannot name the file of another output option");
        }
        if (config_value(cfg, "cyclize_tandem_duplications") == "true")
            return fail("--msa-out, --column-stats and --variable-sites cannot be combined with -c: the final graph then has cycles");
    }
    NamedGraph baseline, given;
    auto load_graph = [&](const std::string& name, const char* what, NamedGraph& into, std::string& err) {
        std::string text;
        if (!read_input(name, text, err)) return false;
        if (!into.load(text.data(), text.size())) { err = std::string("cannot read the ") + what + " graph from " + name + ": not a GFA this tool writes"; return false; }
        if (const std::string* twice = into.repeated_name()) { err = std::string("the ") + what + " graph " + name + " has two paths named " + *twice; return false; }
        if (into.has_cycles()) { err = std::string("the ") + what + " graph " + name + " has cycles: a path meets a node twice"; return false; }
        return true;
    };
    if (agreement) {
        std::string err;
        if (compare_to == "-" || graph_name == "-") return fail("--compare-to and --graph take files, not standard input");
        if (!load_graph(compare_to, "baseline", baseline, err)) return fail(err);
        if (have_graph && !load_graph(graph_name, "given", given, err)) return fail(err);
    }
    if (have_graph) {   // no FASTA, no alignment, nothing on standard output: the given graph against the baseline
        g_level = atoi(config_value(cfg, "logging_level").c_str());
        const int device = devices.empty() ? 0 : devices[0];
        own.ctx = cl_context_create(device);
        if (!own.ctx) return fail("no usable GPU: " + lib_error());
        std::string err;
        if (!write_pair_agreement(own.ctx, given, baseline, pair_agreement, err)) return fail(err);
        log_line(LOG_MINIMAL, "Compared " + graph_name + " with " + compare_to + ", exiting.");
        return 0;
    }
    // --dist-out alone passes the rows through a file of its own next to FILE, which must not be anybody else's
    const std::string dist_tmp = !dist_out.empty() && pair_stats.empty() ? dist_out + ".pair-stats.tmp" : std::string();
    if (!dist_tmp.empty() && std::ifstream(dist_tmp).good()) return fail("--dist-out would overwrite " + dist_tmp + ": remove it or give --pair-stats");

    if (cl_config_validate(cfg)) {
        fprintf(stderr, "error: %s\n", lib_error().c_str());
        print_help(own.defaults);
        return 1;
    }
    g_level = atoi(config_value(cfg, "logging_level").c_str());

    {
        std::string cmd = "Executing command:";
        for (int i = 0; i < argc; ++i) cmd += std::string(" ") + argv[i];
        log_line(LOG_MINIMAL, cmd);
    }
    log_line(LOG_DEBUG, "config file:\n\n" + generate(cfg) + "\n");

    const std::string fasta_name = config_value(cfg, "fasta_name"), tree_name = config_value(cfg, "tree_name");
    std::string fasta_text, newick, err;
    if (!read_input(fasta_name, fasta_text, err)) return fail(err);
    if (!tree_name.empty() && !read_input(tree_name, newick, err)) return fail(err);

    log_line(LOG_BASIC, "Reading input.");
    cl_fasta fa;
    if (cl_parse_fasta(nullptr, fasta_text.data(), fasta_text.size(), &fa)) return fail(lib_error());
    const uint64_t n_sequences = fa.n_sequences;
    const std::vector<std::string> sequence_names(fa.names, fa.names + fa.n_sequences);
    uint64_t n_bases = 0;
    for (uint64_t i = 0; i < fa.n_sequences; ++i) n_bases += fa.lengths[i];
    if (monomer_seed[0]) {   // the templates of --monomers-seed-period: pieces of the first sequence
        cl_monomer_templates seeds;
        if (cl_monomer_seed_templates(fa.sequences, fa.lengths, fa.n_sequences, (uint32_t)monomer_seed[0], (uint32_t)monomer_seed[1], monomer_seed[2],
                                      monomers_params.strands, &seeds)) {
            const std::string why = lib_error();
            cl_fasta_free(&fa);
            return fail("--monomers-seed-period: " + why);
        }
        for (uint64_t m = 0; m < seeds.n_templates; ++m) {
            monomer_templates.names.push_back(seeds.names[m]);
            monomer_templates.bases.push_back(std::string(seeds.templates[m], seeds.lengths[m]));
            monomer_templates.lengths.push_back(seeds.lengths[m]);
        }
        for (size_t m = 0; m < monomer_templates.names.size(); ++m) {
            monomer_templates.name_ptr.push_back(monomer_templates.names[m].c_str());
            monomer_templates.base_ptr.push_back(monomer_templates.bases[m].c_str());
        }
        cl_monomer_templates_free(&seeds);
    }
    cl_fasta_free(&fa);
    if (!dotplot.empty() && n_bases >= (1ull << 30)) return fail("--dotplot takes less than 2^30 bases, the input holds " + std::to_string(n_bases));
    if (!periods.empty() && n_bases >= (1ull << 30)) return fail("--periods takes less than 2^30 bases, the input holds " + std::to_string(n_bases));
    if (!monomers.empty() && n_bases >= (1ull << 30)) return fail("--monomers takes less than 2^30 bases, the input holds " + std::to_string(n_bases));
    if (monomers_only) {   // no alignment, nothing on standard output
        if (n_sequences < 1) return fail("FASTA input from " + (fasta_name == "-" ? std::string("STDIN") : fasta_name) + " contains no sequence");
        own.ctx = cl_context_create(devices.empty() ? 0 : devices[0]);
        if (!own.ctx) return fail("no usable GPU: " + lib_error());
        if (!write_monomers(own.ctx, fasta_text, monomer_templates, monomers_params, monomer_refinement, monomers, monomers_summary, err)) return fail(err);
        log_line(LOG_MINIMAL, "Wrote the monomer decomposition to " + monomers + ", exiting.");
        return 0;
    }
    if (periods_only) {   // no alignment, nothing on standard output
        if (n_sequences < 1) return fail("FASTA input from " + (fasta_name == "-" ? std::string("STDIN") : fasta_name) + " contains no sequence");
        own.ctx = cl_context_create(devices.empty() ? 0 : devices[0]);
        if (!own.ctx) return fail("no usable GPU: " + lib_error());
        if (!write_periods(own.ctx, fasta_text, periods_params, periods_scope, periods, periods_hist, err)) return fail(err);
        log_line(LOG_MINIMAL, "Wrote the period spectra to " + periods + ", exiting.");
        return 0;
    }
    if (dotplot_only) {   // no alignment, nothing on standard output
        if (n_sequences < 1) return fail("FASTA input from " + (fasta_name == "-" ? std::string("STDIN") : fasta_name) + " contains no sequence");
        own.ctx = cl_context_create(devices.empty() ? 0 : devices[0]);
        if (!own.ctx) return fail("no usable GPU: " + lib_error());
        if (!write_dotplot(own.ctx, fasta_text, dotplot_params, dotplot, err)) return fail(err);
        log_line(LOG_MINIMAL, "Wrote the dot plot to " + dotplot + ", exiting.");
        return 0;
    }
    if (n_sequences < 2)
        return fail("FASTA input from " + (fasta_name == "-" ? std::string("STDIN") : fasta_name) + " contains " + std::to_string(n_sequences) +
                    " sequence(s), cannot form an alignment");
    if (pair_positions && n_sequences == 2 && !force_gfa_output)
        return fail("--pair-profile and --pair-events need --force-gfa-output for two sequences: they read the graph that is printed");
    if (agreement && n_sequences == 2 && !force_gfa_output)
        return fail("--compare-to and --pair-agreement need --force-gfa-output for two sequences: they read the graph that is printed");
    if (msa_columns && n_sequences == 2 && !force_gfa_output)
        return fail("--msa-out, --column-stats and --variable-sites need --force-gfa-output for two sequences: they read the graph that is printed");
    if (!dist_out.empty()) {   // the rows name sequences as -A names its files: two names that differ only in '/' and '_' could not be told apart
        std::vector<std::string> flat = sequence_names;
        for (std::string& nm : flat) for (char& c : nm) if (c == '/') c = '_';
        for (size_t a = 0; a < flat.size(); ++a)
            for (size_t b = a + 1; b < flat.size(); ++b)
                if (flat[a] == flat[b]) return fail("--dist-out cannot tell sequences " + sequence_names[a] + " and " + sequence_names[b] + " apart");
    }
    if (tree_name.empty() && !infer_tree && refine_rounds == 0 && n_sequences > 2)
        fprintf(stderr, "warning: it is highly recommended to provide a guide tree (-T) when aligning > 2 sequences\n");

    cl_msa_params mp;
    if (cl_config_msa_params(cfg, &mp)) return fail(lib_error());
    mp.force_gfa_output = force_gfa_output;
    // --dist-out is computed from the rows of the --pair-stats file: without --pair-stats the run writes them next to FILE and the file is removed
    const std::string stats_file = !pair_stats.empty() ? pair_stats : dist_tmp;
    if (!stats_file.empty()) mp.pair_stats_path = stats_file.c_str();
    if (!devices.empty()) {
        mp.devices = devices.data();
        mp.n_devices = (int)devices.size();
    }

    // the device is opened only now: everything above works without one
    const int device = devices.empty() ? 0 : devices[0];
    log_line(LOG_VERBOSE, "Opening GPU " + std::to_string(device) + " with " + std::to_string(mp.n_workers) + " worker context(s).");
    own.ctx = cl_context_create(device);
    if (!own.ctx) return fail("no usable GPU: " + lib_error());

    if (!dotplot.empty()) {
        log_line(LOG_BASIC, "Writing the dot plot.");
        if (!write_dotplot(own.ctx, fasta_text, dotplot_params, dotplot, err)) return fail(err);
    }
    if (!periods.empty()) {
        log_line(LOG_BASIC, "Writing the period spectra.");
        if (!write_periods(own.ctx, fasta_text, periods_params, periods_scope, periods, periods_hist, err)) return fail(err);
    }
    if (!monomers.empty()) {
        log_line(LOG_BASIC, "Writing the monomer decomposition.");
        if (!write_monomers(own.ctx, fasta_text, monomer_templates, monomers_params, monomer_refinement, monomers, monomers_summary, err)) return fail(err);
    }
    if (infer_tree) {   // the tree goes to cl_msa exactly as the text of a -T file would
        log_line(LOG_BASIC, "Inferring a guide tree from k-mer distances.");
        const auto t0 = std::chrono::steady_clock::now();
        char* tree = nullptr;
        uint64_t tree_len = 0;
        if (cl_infer_guide_tree(own.ctx, fasta_text.data(), fasta_text.size(), 21, &tree, &tree_len)) {
            const char* e = cl_last_error(own.ctx);
            return fail(e && *e ? e : lib_error());
        }
        newick.assign(tree, tree_len);
        free(tree);
        char line[128];
        snprintf(line, sizeof(line), "Inferred the guide tree in %.3f s.", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        log_line(LOG_VERBOSE, line);
        log_line(LOG_DEBUG, "guide tree: " + newick);
    }
    bool have_tree = !tree_name.empty() || infer_tree;   // false: cl_msa gets NULL, the sequences in FASTA order
    if (refine_rounds > 0) {   // the refined tree goes to cl_msa exactly as the text of a -T file would
        log_line(LOG_BASIC, "Refining the guide tree from alignment distances.");
        const auto t0 = std::chrono::steady_clock::now();
        int done = 0;
        // One round per call, so that each round's tree can be logged at -v 4: the same rounds, trees and convergence as one call with max_rounds = N
        // (a round depends on the tree text alone), at the price of parsing the FASTA once per round
        for (int r = 0; r < refine_rounds; ++r) {
            char* tree = nullptr;
            uint64_t tree_len = 0;
            int rounds_run = 0, converged = 0;
            if (cl_refine_guide_tree(own.ctx, fasta_text.data(), fasta_text.size(), have_tree ? newick.c_str() : nullptr, &mp, 1, &tree, &tree_len, &rounds_run,
                                     &converged)) {
                const char* e = cl_last_error(own.ctx);
                return fail(e && *e ? e : lib_error());
            }
            if (tree) { newick.assign(tree, tree_len); have_tree = true; }
            free(tree);
            if (rounds_run == 0) break;   // fewer than three sequences: nothing to refine
            ++done;
            log_line(LOG_DEBUG, "guide tree after round " + std::to_string(done) + ": " + newick);
            if (converged) { log_line(LOG_VERBOSE, "The guide tree no longer changes."); break; }
        }
        char line[128];
        snprintf(line, sizeof(line), "Refined the guide tree in %d round(s), %.3f s.", done, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        log_line(LOG_VERBOSE, line);
    }
    if (!tree_out.empty()) {
        FILE* f = fopen(tree_out.c_str(), "wb");
        const std::string text = (have_tree ? newick : std::string()) + "\n";
        const bool written = f && fwrite(text.data(), 1, text.size(), f) == text.size();
        if ((f && fclose(f) != 0) || !written) return fail("could not write the guide tree to " + tree_out);
    }

    log_line(LOG_BASIC, "Aligning " + std::to_string(n_sequences) + " sequences.");
    char* text = nullptr;
    uint64_t len = 0;
    cl_msa_stats st;
    memset(&st, 0, sizeof(st));
    if (cl_msa(own.ctx, fasta_text.data(), fasta_text.size(), have_tree ? newick.c_str() : nullptr, &mp, &text, &len, &st)) {
        const char* e = cl_last_error(own.ctx);
        return fail(e && *e ? e : lib_error());
    }
    const bool written = fwrite(text, 1, len, stdout) == len && fflush(stdout) == 0;
    std::string positions_err;
    const bool positions_ok = !written || !pair_positions || write_pair_positions(own.ctx, text, len, pair_profile, window, pair_events, min_event, positions_err);
    bool agreement_ok = true;
    if (written && positions_ok && agreement) {
        NamedGraph printed;
        agreement_ok = printed.load(text, len) ? write_pair_agreement(own.ctx, printed, baseline, pair_agreement, positions_err)
                                               : (positions_err = "cannot read back the alignment graph", false);
    }
    bool columns_ok = true;
    if (written && positions_ok && agreement_ok && msa_columns)
        columns_ok = write_msa_columns(own.ctx, text, len, msa_out, column_stats, variable_sites, msa_layout, (uint32_t)site_min_minor, (uint32_t)site_max_gaps, positions_err);
    free(text);
    if (!written) return fail("could not write the alignment to standard output");
    if (!positions_ok || !agreement_ok || !columns_ok) return fail(positions_err);
    if (!dist_out.empty()) {
        std::string err;
        const bool ok = write_distances(stats_file, sequence_names, dist_out, err);
        if (pair_stats.empty()) remove(stats_file.c_str());
        if (!ok) return fail(err);
    }

    char line[512];
    snprintf(line, sizeof(line), "%llu merges, score scale %.6g: calibration %.2f s, matches %.2f s, alignment %.2f s, fusion %.2f s",
             (unsigned long long)st.n_merges, st.score_scale, st.calibration_s, st.match_s, st.align_s, st.fuse_s);
    log_line(LOG_VERBOSE, line);
    if (st.n_restarted) log_line(LOG_BASIC, "Loaded " + std::to_string(st.n_restarted) + " subproblem(s) from an earlier run.");
    if (mp.cyclize) log_line(LOG_BASIC, "Merged " + std::to_string(st.n_bonds) + " tandem duplication(s), realigned " + std::to_string(st.n_polished_regions) + " region(s).");
    snprintf(line, sizeof(line), "Run completed successfully in %.2f s, exiting.", st.total_s);
    log_line(LOG_MINIMAL, line);
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
