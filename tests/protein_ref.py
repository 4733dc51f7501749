"""The amino-acid k-mer model (spec D2G-AA: --protein / --protein14 / --protein8 / --protein6), in pure Python / NumPy over the bytes
of a FASTA buffer (test infrastructure; no GPU, nothing of the product in here; held to its own properties by test_protein_ref.py).

An alphabet is a list of residue groups; a residue's code is the position of its group, A the number of groups.  Letters of either
case; any other byte ends a run, and so does a record boundary; runs shorter than k hold no k-mer.  The key of the k-mer with codes
c_0 .. c_{k-1} is sum c_j A^(k-1-j) -- the first residue most significant -- and k is at most the largest with A^k <= 2^64.  There
is no canonical form.  The key then takes the road of a DNA k-mer: masked = wang64(key ^ xormask), and everything downstream is a
function of the per-input (masked key, count) pairs, which the helpers that exist already turn into every expected value
(oph_kmers_ref.closed_form / counts_for, oph_mincount_ref.closed_form, exact_ref, the oracle's BagMinHash over ids and weights).

Two statements of the keys that share nothing but the tables: `run_keys` rolls (NumPy, whole run at once, the way a kernel would);
`run_keys_brute` encodes every k-mer from its letters.
"""
import numpy as np

from filter_ref import records
from minimizer_ref import wang64

DNA, PROTEIN20, PROTEIN_3BIT, PROTEIN_14, PROTEIN_6 = 0, 2, 3, 4, 5        # the reference's python/parse.py:8-23
GROUPS = {
    PROTEIN20: "A C D E F G H I K L M N P Q R S T V W Y",
    PROTEIN_14: "A C D EQ FY G H IV KR LM N P ST W",
    PROTEIN_3BIT: "AST C DHN EKQR FWY G ILMV P",
    PROTEIN_6: "AST CP DEHKNQR FWY G ILMV",
}
NAMES = {DNA: "DNA", PROTEIN20: "PROTEIN20", PROTEIN_3BIT: "PROTEIN_3BIT", PROTEIN_14: "PROTEIN_14", PROTEIN_6: "PROTEIN_6"}
FLAGS = {"--protein": PROTEIN20, "--protein20": PROTEIN20, "--enable-protein": PROTEIN20, "--protein14": PROTEIN_14,
         "--protein8": PROTEIN_3BIT, "--protein6": PROTEIN_6}
ALPHABETS = (PROTEIN20, PROTEIN_14, PROTEIN_3BIT, PROTEIN_6)
LETTERS20 = "ACDEFGHIKLMNPQRSTVWY"
INVALID_LETTERS = "XBZJUO*-"                                                # and every other byte


def size(alphabet):
    return len(GROUPS[alphabet].split())


def max_k(alphabet):
    A, k = size(alphabet), 0
    while A ** (k + 1) <= 2 ** 64:
        k += 1
    return k


def code_table(alphabet):
    """int16[256]: the code of every byte, -1 for one that ends a run"""
    t = np.full(256, -1, np.int16)
    for code, group in enumerate(GROUPS[alphabet].split()):
        for ch in group:
            t[ord(ch)] = t[ord(ch.lower())] = code
    return t


def key_bits(k, alphabet):
    return (size(alphabet) ** k - 1).bit_length()


def runs(seq: bytes, alphabet):
    """the maximal stretches of the alphabet's letters in one record's sequence, as arrays of codes, in order"""
    codes = code_table(alphabet)[np.frombuffer(seq, np.uint8)]
    cut = np.flatnonzero(codes < 0)
    edges = np.concatenate(([-1], cut, [codes.size]))
    return [codes[a + 1:b].astype(np.uint8) for a, b in zip(edges[:-1], edges[1:]) if b - a > 1]


def run_keys(run, k, alphabet):
    """the keys of one run of codes, uint64[len - k + 1], by Horner over k shifted views (exact: every partial sum is below A^k)"""
    n = len(run) - k + 1
    if n <= 0:
        return np.empty(0, np.uint64)
    A = np.uint64(size(alphabet))
    x = np.zeros(n, np.uint64)
    with np.errstate(over="ignore"):
        for j in range(k):
            x = x * A + run[j:j + n].astype(np.uint64)
    return x


def run_keys_brute(letters: bytes, k, alphabet):
    """the same from the LETTERS of a run, one k-mer at a time in Python integers"""
    pos = {ch: i for i, g in enumerate(GROUPS[alphabet].split()) for ch in g}
    A = size(alphabet)
    out = []
    for i in range(len(letters) - k + 1):
        v = 0
        for ch in letters[i:i + k].decode().upper():
            v = v * A + pos[ch]
        out.append(v)
    return out


def seq_keys(seq: bytes, k, alphabet):
    parts = [run_keys(r, k, alphabet) for r in runs(seq, alphabet)]
    return np.concatenate(parts) if parts else np.empty(0, np.uint64)


def fasta_keys(fasta: bytes, k, alphabet):
    """every k-mer of every record of a FASTA buffer, in order (nothing spans records)"""
    parts = [seq_keys(s, k, alphabet) for _, s in records(fasta)]
    return np.concatenate(parts) if parts else np.empty(0, np.uint64)


def masked_counts(keys, xormask=0):
    """the multiset as the exact counter reports it: (masked keys ascending uint64, counts uint32)"""
    if not len(keys):
        return np.empty(0, np.uint64), np.empty(0, np.uint32)
    mk, counts = np.unique(wang64(np.asarray(keys, np.uint64) ^ np.uint64(xormask)), return_counts=True)
    return mk, counts.astype(np.uint32)


def fasta_counts(fasta: bytes, k, alphabet, xormask=0):
    return masked_counts(fasta_keys(fasta, k, alphabet), xormask)


def stream(fastas, k, alphabet, by_record=False):
    """what the packer holds for these inputs: (codes uint8 back to back, run_start, run_len, genome_run_off, k-mers per genome).
    Runs shorter than k are not in the stream.  by_record: every record is its own genome."""
    codes, rs, rl, go, nk = [], [], [], [0], []
    pos = 0
    for fa in fastas:
        recs = records(fa)
        for group in ([[r] for r in recs] if by_record else [recs]):
            tot = 0
            for _, s in group:
                for r in runs(s, alphabet):
                    if len(r) >= k:
                        codes.append(r); rs.append(pos); rl.append(len(r)); pos += len(r); tot += len(r) - k + 1
            go.append(len(rs)); nk.append(tot)
    flat = np.concatenate(codes) if codes else np.empty(0, np.uint8)
    return flat, np.array(rs, np.uint64), np.array(rl, np.uint32), np.array(go, np.uint64), nk


def random_protein(seed, n, letters=LETTERS20):
    rng = np.random.default_rng(seed)
    return np.frombuffer(letters.encode(), np.uint8)[rng.integers(0, len(letters), n)].tobytes()


def fa(seq: bytes, name="p"):
    return b">" + name.encode() + b"\n" + seq + b"\n"


# ---------------------------------------------------------------- the files: the alphabet's name where DNA stands, never .rc_canon
def cache_name(path, S, k, alphabet, seedseed=0, outprefix=None):
    """makedest (src/fastxmerge.cpp:70-120) of a One-Permutation set sketch of an amino-acid input: "." + to_string(rht) at :117"""
    ret = path.split(" ")[0]
    if outprefix:
        ret = outprefix + "/" + ret[ret.rfind("/") + 1:]
    if seedseed:
        ret += ".seed%d" % seedseed
    return ret + ".sketchsize%d.k%d.SetSpace.%s.opss" % (S, k, NAMES[alphabet])


def kmercounts_column(path, S, k, alphabet):
    d = cache_name(path, S, k, alphabet)
    return d[:d.rfind(".")] + ".kmercounts.f64"


def set_name(path, k, alphabet, count_threshold=0):
    """the key file of --set / --countdict: no .sketchsize part (fastxmerge.cpp:85)"""
    ret = path.split(" ")[0] + ".k%d" % k
    if count_threshold:
        ret += ".ct_threshold%d" % count_threshold
    return ret + ".FullMmerSet.%s.kmerset64" % NAMES[alphabet]


def kmer64_header(alphabet, S, k, seedseed=0):
    """[u32 dtype | canon << 8 (canon is 0)][u32 S][u32 k][u32 w = k][u64 seed]"""
    return np.array([alphabet, S, k, k], np.uint32).tobytes() + np.array([seedseed], np.uint64).tobytes()
