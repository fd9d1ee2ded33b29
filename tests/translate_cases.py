"""Inputs and an independent model for the six-frame translation (swg_db_translate, swg_translate_seq).

The model works on STRINGS: a codon is looked up by its three letters in the seven NCBI tables typed in below, and the
reverse frames come from an explicitly reverse-complemented string.  Nothing here reads the library's tables or bit
planes.  Sequences are generated, so no fixture is needed."""
import numpy as np

BASES = "TCAG"
# NCBI genetic codes, the amino acids of TTT, TTC, TTA, TTG, TCT, ... GGG (TCAG order)
TABLES = {
    1: "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    2: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG",
    3: "FFLLSSSSYY**CCWWTTTTPPPPHHQQRRRRIIMMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    4: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    5: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSSSVVVVAAAADDEEGGGG",
    6: "FFLLSSSSYYQQCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    11: "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
}
# a caller-made table: code 1 with the amino acids rotated (every entry differs from code 1's), and no stop at all
CUSTOM = "".join("ACDEFGHIKLMNPQRSTVWY"[("ACDEFGHIKLMNPQRSTVWY".index(a) + 7) % 20] if a != "*" else "K" for a in TABLES[1])
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A"}
ALL_CODONS = [a + b + c for a in BASES for b in BASES for c in BASES]


def letter_index(ch):
    """The library's residue index of a letter: its position in the alphabet, '*' = 31."""
    return 31 if ch == "*" else ord(ch.upper()) - ord("A") + 1


def indices(s):
    return np.array([letter_index(c) for c in s], dtype=np.int8)


def table_indices(letters):
    return indices(letters)


def revcomp(s):
    """The reverse complement; a letter that is no base stays what it is (it is no base on either strand)."""
    return "".join(COMPLEMENT.get(c, c) for c in reversed(s.upper()))


def _frame(s, f, letters, unknown):
    codon = {c: letters[k] for k, c in enumerate(ALL_CODONS)}
    out = []
    for a in range(f, len(s) - 2, 3):
        c = s[a:a + 3].replace("U", "T")
        out.append(codon.get(c, unknown))
    return "".join(out)


def model(s, letters=TABLES[1], unknown="X"):
    """The six frames of the nucleotide string s as strings of amino-acid letters."""
    s = s.upper()
    rc = revcomp(s)
    return [_frame(s, f, letters, unknown) for f in range(3)] + [_frame(rc, f, letters, unknown) for f in range(3)]


def model_counts(seqs, letters=TABLES[1]):
    """(codons, stops, codons with a non-base) over the six frames of every sequence."""
    codons = stops = unknown = 0
    for s in seqs:
        for fr in model(s, letters, unknown="?"):
            codons += len(fr)
            stops += fr.count("*")
            unknown += fr.count("?")
    return codons, stops, unknown


def consumed(L, frame):
    """For each residue of `frame` of a sequence of L nucleotides: the set of forward-strand positions its codon read."""
    f = frame % 3
    out = []
    for a in range(f, L - 2, 3):
        pos = (a, a + 1, a + 2)
        out.append(frozenset(pos) if frame < 3 else frozenset(L - 1 - p for p in pos))
    return out


def codon_cases():
    """Every one of the 64 codons in every one of the six frames of some case: all 64 end to end, the same with one and
    two bases in front, and the reverse complements of the three."""
    run = "".join(ALL_CODONS)
    cases = {"codons+0": run, "codons+1": "G" + run, "codons+2": "CA" + run}
    for k in list(cases):
        cases[k + "_rc"] = revcomp(cases[k])
    return cases


def random_nt(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), size=n)) if n else ""


def structural_cases(T, seed=20260001):
    """The GPU test's database: name -> nucleotide string.  T: codons per tile of the kernel."""
    rng = np.random.default_rng(seed)
    cases = {}
    for L in range(0, 15):                                   # every remainder mod 3 and mod 12, frames of 0 residues, all partial codon
        cases["len_%02d" % L] = random_nt(rng, L)
    cases.update(codon_cases())
    for d in range(-13, 14):                                 # a tile seam at every phase of the frame offset and of the output dword
        cases["tile_%+03d" % d] = random_nt(rng, 3 * T + d)
    cases["tile_x2_+7"] = random_nt(rng, 2 * 3 * T + 7)
    cases["tile_x3_+5"] = random_nt(rng, 3 * 3 * T + 5)
    for pos in range(3):                                     # a non-base at each codon position next to a tile seam and in the last codon
        for where in ("seam", "last"):
            for L in (3 * T + 9, 3 * T + 10, 3 * T + 11):
                s = list(random_nt(rng, L))
                at = (3 * T - 3 + pos) if where == "seam" else (L - 3 - (L % 3) + pos)
                s[at] = "N"
                s[L - 1 - at] = "R"                          # (the same place seen from the other strand)
                s[3 * T + pos] = "*"
                cases["nonbase_%s_%d_%d" % (where, pos, L)] = "".join(s)
    for i in range(90):                                      # short sequences back to back: several to a 64-byte line
        cases["short_%02d" % i] = random_nt(rng, 1 + i % 20, "ACGTUN")
    for i in range(40):                                      # equal lengths, and lengths 1 and 2 apart: frames that tie in length
        cases["tie_%02d" % i] = random_nt(rng, 60 + i % 3)
    for i in range(30):                                      # bulk
        cases["bulk_%02d" % i] = random_nt(rng, int(rng.integers(50, 901)), "ACGT" * 8 + "NU")
    return cases


def flat_of(seqs):
    """Sequences (strings or index arrays) -> (flat int8, offsets uint64)."""
    arrs = [indices(s) if isinstance(s, str) else np.asarray(s, dtype=np.int8) for s in seqs]
    off = np.zeros(len(arrs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([a.size for a in arrs])
    flat = np.concatenate(arrs) if arrs and int(off[-1]) else np.zeros(0, dtype=np.int8)
    return np.ascontiguousarray(flat, dtype=np.int8), off


def back_translate(rng, protein, letters=TABLES[1]):
    """A nucleotide string whose frame 0 under `letters` spells `protein`: each codon drawn among the synonyms."""
    syn = {}
    for k, a in enumerate(letters):
        syn.setdefault(a, []).append(ALL_CODONS[k])
    return "".join(syn[a][int(rng.integers(len(syn[a])))] for a in protein)


def planted(seed=20260002, lq=120, letters=TABLES[1]):
    """A protein query and six nucleotide records that each hold its back-translation in one known frame at a known place.
    -> dict(query letters, records [strings], plants [(record, frame, nt_begin, nt_end)]): the interval is 0-based and
    half-open on the forward strand.  The flanks are stop-rich (TAA TAG TGA runs are avoided by chance only, so they are
    drawn from AT-only letters, which never spell the query)."""
    rng = np.random.default_rng(seed)
    aas = "ACDEFGHIKLMNPQRSTVWY"
    query = "".join(rng.choice(list(aas), size=lq))
    records, plants = [], []
    for frame in range(6):
        f = frame % 3
        gene = back_translate(rng, query, letters)
        left = 3 * int(rng.integers(5, 40)) + f              # the gene starts at offset f mod 3 of its strand
        right = int(rng.integers(20, 90))
        strand = random_nt(rng, left, "AT") + gene + random_nt(rng, right, "AT")
        L = len(strand)
        if frame < 3:
            records.append(strand)
            plants.append((frame, frame, left, left + len(gene)))
        else:
            records.append(revcomp(strand))
            plants.append((frame, frame, L - left - len(gene), L - left))
    return dict(query=query, records=records, plants=plants)
