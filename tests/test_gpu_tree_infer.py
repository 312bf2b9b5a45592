"""--infer-tree on the device: the k-mer spectra and pair sums of cl_kmer_distances_compute (tree_kernels.hip) against a numpy restatement,
exactly — up to 200 sequences: more than the 16 384 workgroups of pair_shared_kernel have tiles, so its loop over the tiles runs again, and
k = 31, 30, 29 and 11 form spectra groups of 4, 16, 64 and 200 sequences, the last two with more than one workgroup of seq_bounds_kernel —;
the distances against math.log to the bit; the topology of an evolved family; the command line end to end.  CLI runs are fresh
child processes with their own time limits, one at a time; after a child that ends by a signal or times out none is started."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests.test_tree_infer import splits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign")
PAIR_TILE = 2048   # merged items per pair tile of tree_kernels.hip ("Guide tree inference")
_LUT = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _LUT[ord(_c)] = _LUT[ord(_c.lower())] = _i
_faulted = []


def spectrum(seq, k):
    """(sorted distinct keys, counts) of the forward-strand k-mers of seq: windows of k characters all from ACGTacgt, first base most significant"""
    code = _LUT[np.frombuffer(seq.encode(), np.uint8)]
    w = len(code) - k + 1
    if w <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    bad = np.concatenate([[0], np.cumsum(code > 3)])
    ok = bad[k:k + w] == bad[:w]
    key = np.zeros(w, np.uint64)
    for j in range(k):
        key = (key << np.uint64(2)) | (code[j:j + w] & 3).astype(np.uint64)
    return np.unique(key[ok], return_counts=True)


def restated(seqs, k):
    spec = [spectrum(s, k) for s in seqs]
    n = len(seqs)
    total = np.array([int(c.sum()) for _, c in spec], np.uint64)
    shared = np.zeros((n, n), np.uint64)
    for i in range(n):
        shared[i, i] = total[i]
        for j in range(i + 1, n):
            _, a, b = np.intersect1d(spec[i][0], spec[j][0], assume_unique=True, return_indices=True)
            shared[i, j] = shared[j, i] = int(np.minimum(spec[i][1][a], spec[j][1][b]).sum())
    return total, shared, spec


def py_distance(shared, total, k):
    n = len(total)
    out = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            s, uni = int(shared[i, j]), int(total[i]) + int(total[j]) - int(shared[i, j])
            J = s / uni if uni else 0.0
            out[i, j] = 1.0 if J == 0 else 0.0 if J == 1 else min(1.0, -math.log(2 * J / (1 + J)) / k)
    return out


def check(ctx, seqs, k):
    total, shared, distance = capi.kmer_distances(ctx, seqs, k=k)
    want_total, want_shared, spec = restated(seqs, k)
    assert np.array_equal(total, want_total)
    assert np.array_equal(shared, want_shared)
    assert np.array_equal(distance.view(np.uint64), py_distance(want_shared, want_total, k).view(np.uint64))
    return spec


def messy_sequences(seed):
    rng = random.Random(seed)
    alphabet = "ACGTACGTACGTacgtNRYKMacgtn"
    out = ["", "A", "ACG", "N" * 40, "acgtNNacgt" * 7]
    base = "".join(rng.choice("ACGT") for _ in range(6000))
    for i in range(6):
        s = list(base[rng.randrange(0, 500):rng.randrange(3000, 6000)])
        for _ in range(len(s) // 50):
            s[rng.randrange(len(s))] = rng.choice(alphabet)
        out.append("".join(s))
    out.append("".join(rng.choice(alphabet) for _ in range(9000)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 15, 21, 31])
def test_gpu_spectra_of_messy_sequences(gpu_ctx, k):
    """N, IUPAC letters, lowercase, empty sequences and sequences shorter than k"""
    check(gpu_ctx, messy_sequences(k), k)


@pytest.fixture(scope="module")
def hor12():
    return synth.hor_sequences(41, 200000, 12)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 15, 21, 31])
def test_gpu_spectra_of_hor_arrays(gpu_ctx, hor12, k):
    """12 x 200 kbp HOR arrays; at k = 31 the sequence index leaves room for groups of four, and a pair computed alone gives the same sums"""
    check(gpu_ctx, hor12, k)
    if k == 31:
        alone = capi.kmer_distances(gpu_ctx, [hor12[2], hor12[9]], k=k)
        together = capi.kmer_distances(gpu_ctx, hor12, k=k)
        assert int(alone[1][0, 1]) == int(together[1][2, 9]) and int(alone[0][1]) == int(together[0][9])


def straddles(spec_a, spec_b):
    """equal keys of a pair whose copies lie on either side of a tile edge of the merge path (list a first on equal keys)"""
    ka, kb = spec_a[0], spec_b[0]
    pos_a = np.arange(len(ka)) + np.searchsorted(kb, ka, side="left")
    common = np.isin(ka, kb, assume_unique=True)
    return int(np.count_nonzero(common & ((pos_a + 1) % PAIR_TILE == 0)))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [15, 21, 31])
def test_gpu_shared_keys_across_tile_edges(gpu_ctx, k):
    """distinct lists at and around multiples of the tile size, cut from one random text with a few changes, so that many equal keys sit
    next to each other in the merge path and some of them on either side of a tile edge"""
    rng = random.Random(1000 + k)
    base = [rng.choice("ACGT") for _ in range(5 * PAIR_TILE + 100)]
    seqs = []
    for distinct in (1, PAIR_TILE - 1, PAIR_TILE, PAIR_TILE + 1, 2 * PAIR_TILE - 1, 2 * PAIR_TILE, 2 * PAIR_TILE + 1, 3 * PAIR_TILE + 7,
                     PAIR_TILE // 2, 4 * PAIR_TILE):
        off = rng.randrange(0, 64)
        s = base[off:off + distinct + k - 1]
        for _ in range(rng.randrange(0, 3)):
            s[rng.randrange(len(s))] = rng.choice("ACGT")
        seqs.append("".join(s))
    spec = check(gpu_ctx, seqs, k)
    assert any(len(spec[i][0]) % PAIR_TILE == 0 for i in range(len(seqs)))
    assert sum(straddles(spec[i], spec[j]) for i in range(len(seqs)) for j in range(i + 1, len(seqs))) > 0


@pytest.fixture(scope="module")
def family200():
    return family200_sequences()


def family200_sequences():
    """200 sequences: mutated copies of 100 to 400 bases of one 300-base ancestor; an empty one, one shorter than any k of the test and one of
    N only at 0, 3, 4, 15, 16, 63, 64 and 199 — the first and last places of the spectra groups of k = 31 (4 sequences), 30 (16) and 29 (64)
    —; and a 20 kbp sequence at 1 and at 198, whose pairs have ten and twenty tiles where the others have one"""
    rng = random.Random(200)
    anc = [rng.choice("ACGT") for _ in range(300)]
    seqs = []
    for _ in range(200):
        s = [c if rng.random() > 0.05 else rng.choice("ACGT") for c in anc]
        n = rng.randrange(100, 401)
        seqs.append("".join(s[:n] + [rng.choice("ACGT") for _ in range(n - 300)]))
    for i, s in zip((0, 3, 4, 15, 16, 63, 64, 199), ("", "ACGTA", "N" * 150, "ACGTACGTAC", "", "N" * 40, "ACG", "")):
        seqs[i] = s
    for i in (1, 198):
        seqs[i] = "".join(rng.choice("ACGT") for _ in range(20000))
    return seqs


@pytest.mark.gpu
@pytest.mark.parametrize("k", [11, 29, 30, 31])
def test_gpu_more_tiles_than_workgroups_and_every_group_size(gpu_ctx, family200, k):
    """19 900 pairs, more than 16 384 of them with a tile: pair_shared_kernel's workgroups go round their loop again, reusing sb, split and
    part, early and late ones with a many-tile pair among one-tile pairs.  k = 31, 30 and 29 form groups of 4, 16 and 64 sequences — the
    sequences without a k-mer are the first or last of a group —, k = 11 one group of 200: seq_bounds_kernel runs two and four workgroups"""
    spec = check(gpu_ctx, family200, k)
    sizes = np.array([len(keys) for keys, _ in spec])
    assert np.count_nonzero(sizes) == 192
    both = np.triu(np.outer(sizes > 0, sizes > 0), 1)
    tiles = -(-(sizes[:, None] + sizes[None, :]) // PAIR_TILE)
    assert int(both.sum()) == 18336 and int(tiles[both].sum()) > 16384
    assert int(tiles[1, 198]) >= 10 and int(tiles[1, 5]) >= 5 and int(tiles[5, 150]) == 1
    if k == 29:
        together = capi.kmer_distances(gpu_ctx, family200, k=k)
        for a, b in ((1, 198), (5, 150)):
            alone = capi.kmer_distances(gpu_ctx, [family200[a], family200[b]], k=k)
            assert int(alone[1][0, 1]) == int(together[1][a, b]) and alone[0].tolist() == [int(together[0][a]), int(together[0][b])]


def evolve_family(seed=3, length=100000):
    """((((0,1),(2,3)),((4,5),(6,7))) from one HOR array: 0.003 per internal branch, 0.002 per leaf branch"""
    rng = random.Random(seed)
    root = synth.hor_sequences(seed, length, 1)[0]

    def down(s, r):
        return "".join(synth._mut_track(rng, s, r)[0])

    leaves = []
    for a in (down(root, 0.003), down(root, 0.003)):
        for b in (down(a, 0.003), down(a, 0.003)):
            leaves += [down(b, 0.002), down(b, 0.002)]
    return leaves


@pytest.mark.gpu
def test_gpu_inferred_tree_has_the_true_bipartitions(gpu_ctx):
    seqs = evolve_family()
    names = ["leaf%d" % i for i in range(8)]
    fasta = "".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs))
    text = capi.infer_guide_tree(gpu_ctx, fasta)
    # the true bipartitions, each as the side without names[0] (as splits() gives them)
    want = {frozenset(names[i] for i in range(8) if (i in side) != (0 in side)) for side in ([0, 1], [2, 3], [4, 5], [6, 7], [4, 5, 6, 7])}
    assert splits(text, names) == want, text
    _, _, distance = capi.kmer_distances(gpu_ctx, seqs)
    assert text == capi.neighbor_joining_newick(distance, names)
    assert max(distance[0, 1], distance[2, 3], distance[4, 5], distance[6, 7]) < min(distance[0, 4], distance[1, 7], distance[3, 5])


@pytest.mark.gpu
def test_gpu_bad_k_is_refused(gpu_ctx):
    for k in (0, 32):
        with pytest.raises(capi.ClError) as e:
            capi.kmer_distances(gpu_ctx, ["ACGT", "ACGA"], k=k)
        assert e.value.code == -1
    with pytest.raises(capi.ClError):
        capi.kmer_distances(gpu_ctx, ["ACGT"], k=3)
    with pytest.raises(capi.ClError):
        capi.infer_guide_tree(gpu_ctx, ">a\nACGT\n>a\nACGA\n")


def run(args, cwd, timeout=600):
    if _faulted:
        pytest.fail("an earlier child of this module ended abnormally (%s): no further GPU process is started" % _faulted[0])
    try:
        r = subprocess.run([BIN] + [str(a) for a in args], cwd=str(cwd), capture_output=True, timeout=timeout, stdin=subprocess.DEVNULL)
    except subprocess.TimeoutExpired:
        _faulted.append("time limit of %d s" % timeout)
        raise
    if r.returncode < 0:
        _faulted.append("signal %d" % -r.returncode)
        pytest.fail("killed by signal %d: %s" % (-r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


@pytest.mark.gpu
def test_gpu_cli_infer_tree(tmp_path):
    """--infer-tree --tree-out t.nwk prints what -T t.nwk prints; the tree is the same from run to run; a -S run and a -R run with
    --infer-tree find the same subproblem files"""
    seqs = synth.hor_sequences(17, 6000, 5, seq_div=0.01, hor_div=0.03)
    (tmp_path / "in.fa").write_text("".join(">seq%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    first = run(["--infer-tree", "--tree-out", "t.nwk", "-v", "4", "in.fa"], tmp_path)
    tree = (tmp_path / "t.nwk").read_text()
    assert tree.endswith(";\n") and tree.count("\n") == 1
    err = first.stderr.decode()
    assert "warning" not in err and ("guide tree: " + tree[:-1]) in err and "Inferred the guide tree in" in err
    given = run(["-T", "t.nwk", "in.fa"], tmp_path)
    assert first.stdout == given.stdout and first.stdout.startswith(b"H\t")
    run(["--infer-tree", "--tree-out", "t2.nwk", "-v", "0", "in.fa"], tmp_path)
    assert (tmp_path / "t2.nwk").read_text() == tree
    sp = run(["--infer-tree", "-S", "sp", "in.fa"], tmp_path)
    again = run(["--infer-tree", "-S", "sp", "-R", "in.fa"], tmp_path)
    assert again.stdout == sp.stdout == first.stdout
    loaded = [ln for ln in again.stderr.decode().split("\n") if "subproblem(s) from an earlier run" in ln]
    assert len(loaded) == 1 and int(loaded[0].split("Loaded ")[1].split()[0]) > 0


@pytest.mark.gpu
def test_gpu_cli_infer_tree_two_sequences(tmp_path):
    """two sequences: the CIGAR line of a plain run; the tree is still written"""
    seqs = synth.hor_sequences(18, 5000, 2)
    (tmp_path / "in.fa").write_text("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    inferred = run(["--infer-tree", "--tree-out", "t.nwk", "-v", "0", "in.fa"], tmp_path)
    plain = run(["-v", "0", "in.fa"], tmp_path)
    assert inferred.stdout == plain.stdout and inferred.stderr == b""
    assert (tmp_path / "t.nwk").read_text().startswith('("s0":')
