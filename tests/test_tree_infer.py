"""The host half of --infer-tree without a device: neighbor joining, the midpoint root and the Newick text of cl_neighbor_joining_newick
(cl_tree_api.cpp) against the textbook example, against the topology of additive matrices, and character for character against the Python
restatement below; the command line's refusals of the tree options."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign")


# ---- the restatement: every number and tie-break of the tree, in Python floats -------------------------------------------------------------

def _nonneg(x):
    return x if x > 0 else 0.0


def nj_newick(dist, names):
    """neighbor joining (Studier-Keppler Q, first strict minimum in list order), midpoint root, Newick with '%g' lengths"""
    n = len(names)
    d = {(i, j): float(dist[i][j]) for i in range(n) for j in range(n)}
    adj = {i: [] for i in range(n)}

    def edge(a, b, ln):
        adj.setdefault(a, []).append((b, ln))
        adj.setdefault(b, []).append((a, ln))

    active, nxt = list(range(n)), n
    while len(active) > 2:
        r = len(active)
        R = []
        for x in range(r):
            s = 0.0
            for y in range(r):
                if y != x:
                    s += d[active[x], active[y]]
            R.append(s)
        best = None
        for x in range(r):
            for y in range(x + 1, r):
                q = (r - 2) * d[active[x], active[y]] - R[x] - R[y]
                if best is None or q < best[0]:
                    best = (q, x, y)
        _, bx, by = best
        a, b, u = active[bx], active[by], nxt
        nxt += 1
        dab = d[a, b]
        la = dab / 2 + (R[bx] - R[by]) / (2 * (r - 2))
        lb = dab - la
        for c in active:
            if c != a and c != b:
                d[u, c] = d[c, u] = (d[a, c] + d[b, c] - dab) / 2
        edge(u, a, _nonneg(la))
        edge(u, b, _nonneg(lb))
        active = [c for c in active if c != a and c != b] + [u]
    edge(active[0], active[1], _nonneg(d[active[0], active[1]]))

    def walk(p):
        dist_p, toward, stack = {p: 0.0}, {p: p}, [p]
        while stack:
            u = stack.pop()
            for v, ln in adj[u]:
                if v not in toward:
                    toward[v] = u
                    dist_p[v] = dist_p[u] + ln
                    stack.append(v)
        return dist_p, toward

    best = None
    for p in range(n):
        dp, _ = walk(p)
        for q in range(p + 1, n):
            if best is None or dp[q] > best[0]:
                best = (dp[q], p, q)
    longest, p, q = best
    _, toward = walk(p)
    path = [q]
    while path[-1] != p:
        path.append(toward[path[-1]])
    path.reverse()
    half, acc, root = longest / 2, 0.0, None
    for u, v in zip(path, path[1:]):
        if acc == half and u >= n:
            root = u
            break
        ln = [x for w, x in adj[u] if w == v][0]
        if acc + ln > half or acc == half:
            root = nxt
            adj[u] = [(w, x) for w, x in adj[u] if w != v]
            adj[v] = [(w, x) for w, x in adj[v] if w != u]
            edge(root, u, half - acc)
            edge(root, v, ln - (half - acc))
            break
        acc += ln

    def text(u, parent, up):
        kids = [(w, x) for w, x in adj[u] if w != parent]
        if kids:
            kids.sort(key=lambda wx: min_leaf(wx[0], u))
            s = "(" + ",".join(text(w, u, x) for w, x in kids) + ")"
        else:
            s = '"%s"' % names[u]
        return s if parent is None else s + ":" + "%g" % up

    def min_leaf(u, parent):
        if u < n:
            return u
        return min(min_leaf(w, u) for w, _ in adj[u] if w != parent)

    return text(root, None, None) + ";"


# ---- a small Newick reader for the checks ----------------------------------------------------------------------------------------------------

def parse_newick(s):
    """-> (children: {node: [(child, length)]}, label: {leaf node: name}, root)"""
    assert s.endswith(";")
    kids, label, pos, count = {}, {}, [0], [0]

    def node():
        me = count[0]
        count[0] += 1
        kids[me] = []
        if s[pos[0]] == "(":
            pos[0] += 1
            while True:
                c, ln = node()
                kids[me].append((c, ln))
                if s[pos[0]] == ",":
                    pos[0] += 1
                    continue
                assert s[pos[0]] == ")"
                pos[0] += 1
                break
        else:
            assert s[pos[0]] == '"'
            end = s.index('"', pos[0] + 1)
            label[me] = s[pos[0] + 1:end]
            pos[0] = end + 1
        ln = None
        if s[pos[0]] == ":":
            end = pos[0] + 1
            while s[end] not in ",);":
                end += 1
            ln = float(s[pos[0] + 1:end])
            pos[0] = end
        return me, ln

    root, ln = node()
    assert ln is None and s[pos[0]:] == ";"
    return kids, label, root


def splits(newick, names):
    """the non-trivial bipartitions of the unrooted tree, each as the frozenset of names on the side without names[0]"""
    kids, label, root = parse_newick(newick)
    every = frozenset(names)
    out = set()

    def below(u):
        if u in label:
            return frozenset([label[u]])
        return frozenset().union(*[below(c) for c, _ in kids[u]])

    for u in kids:
        if u == root:
            continue
        side = below(u)
        if names[0] in side:
            side = every - side
        if 1 < len(side) < len(names) - 1:
            out.add(side)
    return out


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------

WIKI = ["a", "b", "c", "d", "e"]
WIKI_D = [[0, 5, 9, 9, 8], [5, 0, 10, 10, 9], [9, 10, 0, 8, 7], [9, 10, 8, 0, 3], [8, 9, 7, 3, 0]]


def test_saitou_nei_example():
    """the worked example of neighbor joining (Wikipedia, "Neighbor joining"): a:2, b:3, c:4, d:2, e:1, internal edges 3 and 2"""
    text = capi.neighbor_joining_newick(np.array(WIKI_D, float), WIKI)
    assert text == nj_newick(WIKI_D, WIKI)
    kids, label, root = parse_newick(text)
    # undirected edges; the root (degree 2 on an edge) is folded into one edge of the unrooted tree
    adj = {}
    for u, cs in kids.items():
        for c, ln in cs:
            adj.setdefault(u, []).append((c, ln))
            adj.setdefault(c, []).append((u, ln))
    assert len(adj[root]) == 2
    (x, lx), (y, ly) = adj[root]
    adj[x] = [(w, ln) for w, ln in adj[x] if w != root] + [(y, lx + ly)]
    adj[y] = [(w, ln) for w, ln in adj[y] if w != root] + [(x, lx + ly)]
    del adj[root]
    pendant = {label[u]: adj[u][0][1] for u in label}
    for name, want in dict(a=2, b=3, c=4, d=2, e=1).items():
        assert abs(pendant[name] - want) < 1e-12, (name, pendant)
    internal = sorted(ln for u in adj if u not in label for w, ln in adj[u] if w not in label and u < w)
    assert len(internal) == 2 and all(abs(g - w) < 1e-12 for g, w in zip(internal, [2, 3]))
    # the longest leaf-to-leaf path is b-c (10); the root sits on it, 5 from b
    leaf = {v: k for k, v in label.items()}

    def depth(target):
        def go(u, acc):
            if u == target:
                return acc
            for c, ln in kids[u]:
                r = go(c, acc + ln)
                if r is not None:
                    return r
            return None
        return go(root, 0.0)

    assert abs(depth(leaf["b"]) - 5) < 1e-12 and abs(depth(leaf["c"]) - 5) < 1e-12
    assert [label.get(c) for c, _ in kids[root]] == [None, None]


def random_binary_tree(rng, n):
    """(edges [(u, v, length)], leaves 0..n-1): random joins of a pool of subtrees"""
    pool, edges, nxt = list(range(n)), [], n
    while len(pool) > 2:
        a, b = rng.sample(pool, 2)
        pool.remove(a)
        pool.remove(b)
        edges += [(nxt, a, rng.uniform(0.05, 1.0)), (nxt, b, rng.uniform(0.05, 1.0))]
        pool.append(nxt)
        nxt += 1
    edges.append((pool[0], pool[1], rng.uniform(0.05, 1.0)))
    return edges


def tree_distances(edges, n):
    adj = {}
    for u, v, ln in edges:
        adj.setdefault(u, []).append((v, ln))
        adj.setdefault(v, []).append((u, ln))
    D = np.zeros((n, n))
    for p in range(n):
        dist, stack = {p: 0.0}, [p]
        while stack:
            u = stack.pop()
            for v, ln in adj[u]:
                if v not in dist:
                    dist[v] = dist[u] + ln
                    stack.append(v)
        for q in range(n):
            D[p, q] = dist[q]
    return np.minimum(D, D.T)   # (exactly symmetric)


def true_splits(edges, n, names):
    adj = {}
    for u, v, _ in edges:
        adj.setdefault(u, []).append(v)
        adj.setdefault(v, []).append(u)
    out = set()
    for u, v, _ in edges:
        side, stack = {v}, [v]
        while stack:
            x = stack.pop()
            for y in adj[x]:
                if y != u and y not in side:
                    side.add(y)
                    stack.append(y)
        s = frozenset(names[x] for x in side if x < n)
        if names[0] in s:
            s = frozenset(names) - s
        if 1 < len(s) < n - 1:
            out.add(s)
    return out


@pytest.mark.parametrize("seed", range(12))
def test_additive_matrices_give_their_tree(seed):
    rng = random.Random(seed)
    n = rng.randint(3, 40)
    names = ["t%d" % i for i in range(n)]
    edges = random_binary_tree(rng, n)
    D = tree_distances(edges, n)
    text = capi.neighbor_joining_newick(D, names)
    assert splits(text, names) == true_splits(edges, n, names)   # Robinson-Foulds distance 0
    assert text == nj_newick(D, names)


@pytest.mark.parametrize("seed", range(20))
def test_non_additive_matrices_match_the_restatement(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 30))
    if seed % 4 == 0:
        A = rng.integers(1, 4, size=(n, n)).astype(float)   # small integers: many ties in Q and in the longest path
    elif seed % 4 == 1:
        A = rng.random((n, n)) * 1e-3
    else:
        A = rng.random((n, n))
    D = np.triu(A, 1)
    D = D + D.T
    names = ["s%d_%d" % (seed, i) for i in range(n)]
    assert capi.neighbor_joining_newick(D, names) == nj_newick(D, names)


@pytest.mark.parametrize("n", [2, 3, 4, 7, 16])
@pytest.mark.parametrize("value", [0.0, 0.25, 1.0])
def test_all_equal_distances_match_the_restatement(n, value):
    D = np.full((n, n), value)
    np.fill_diagonal(D, 0.0)
    names = ["x%d" % i for i in range(n)]
    text = capi.neighbor_joining_newick(D, names)
    assert text == nj_newick(D, names)
    assert '"-' not in text and ":-" not in text and text.endswith(";")
    for i in range(n):
        assert text.count('"x%d"' % i) == 1


def test_two_sequences_root_in_the_middle():
    assert capi.neighbor_joining_newick(np.array([[0, 0.5], [0.5, 0]]), ["p", "q"]) == '("p":0.25,"q":0.25);'
    assert capi.neighbor_joining_newick(np.zeros((2, 2)), ["p", "q"]) == '("p":0,"q":0);'


def test_newick_feeds_the_plan():
    """the inferred text is a tree cl_msa_plan_create takes: every name a leaf, n - 1 merges"""
    rng = random.Random(5)
    names = ["chr%d" % i for i in range(9)]
    D = tree_distances(random_binary_tree(rng, 9), 9)
    leaves, merges = capi.msa_plan(capi.neighbor_joining_newick(D, names), names)
    assert sorted(leaves) == list(range(9)) and len(merges) == 8


@pytest.mark.parametrize("case", ["one", "duplicate", "quote", "asymmetric", "nan", "inf", "diagonal"])
def test_bad_input_is_refused(case):
    D = np.array(WIKI_D, float)
    names = list(WIKI)
    if case == "one":
        D, names = np.zeros((1, 1)), ["a"]
    elif case == "duplicate":
        names[3] = "a"
    elif case == "quote":
        names[2] = 'c"x'
    elif case == "asymmetric":
        D[1, 2] += 1e-9
    elif case == "nan":
        D[0, 4] = D[4, 0] = math.nan
    elif case == "inf":
        D[0, 4] = D[4, 0] = math.inf
    elif case == "diagonal":
        D[2, 2] = 1e-300
    with pytest.raises(capi.ClError) as e:
        capi.neighbor_joining_newick(D, names)
    assert e.value.code == -1


def run_cli(args, cwd):
    r = subprocess.run([BIN] + [str(a) for a in args], cwd=str(cwd), capture_output=True, timeout=60, stdin=subprocess.DEVNULL)
    assert r.returncode >= 0, "killed by signal %d" % -r.returncode
    return r


def test_cli_refuses_bad_tree_option_combinations(tmp_path):
    """before the FASTA is read or a device is opened: status 1, one error line, nothing on standard output"""
    (tmp_path / "in.fa").write_text(">a\nACGT\n>b\nACGA\n>c\nACGG\n")
    (tmp_path / "t.nwk").write_text('("a","b","c");\n')
    (tmp_path / "c.yaml").write_text("---\ntree_name: t.nwk\nfasta_name: in.fa\n")
    for args in (["--infer-tree", "-T", "t.nwk", "in.fa"], ["-T", "t.nwk", "--infer-tree", "in.fa"], ["--infer-tree", "-C", "c.yaml"],
                 ["--tree-out", "out.nwk", "in.fa"], ["--tree-out", "out.nwk", "-T", "t.nwk", "in.fa"]):
        r = run_cli(args, tmp_path)
        assert r.returncode == 1 and r.stdout == b"", args
        assert r.stderr.decode().startswith("error: ") and r.stderr.count(b"\n") == 1, (args, r.stderr)
        assert not (tmp_path / "out.nwk").exists()


def test_cli_tree_options_leave_generate_config_alone():
    plain = run_cli(["-G"], ROOT)
    assert run_cli(["--infer-tree", "--tree-out", "x.nwk", "-G"], ROOT).stdout == plain.stdout
    assert b"--infer-tree" in run_cli(["-h"], ROOT).stderr
