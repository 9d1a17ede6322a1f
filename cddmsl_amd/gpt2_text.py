"""GPT-2 byte-level tokens, both ways, as ``GPT2Tokenizer`` does it.

Decoding (ids -> text): ids map to vocabulary strings, the byte-to-unicode table is undone, and the bytes are decoded as UTF-8 with
``errors="replace"``.  Encoding (text -> ids, what mapper training needs for its captions): GPT-2's split pattern cuts the text into
pre-tokens, each is spelt in byte symbols and merged by byte-pair encoding with the ranks of ``vocab.bpe``.  The vocabulary is
GPT-2's ``encoder.json`` / ``vocab.json`` (token string -> id) and ``vocab.bpe`` / ``merges.txt``; neither ships with the repository.
Decoding alone needs no merges file."""
import json
from typing import Dict, Iterable, List, Optional, Tuple

from .clip_text import byte_symbols

# GPT-2's pre-tokeniser (openai/gpt-2 encoder.py): contractions, letter runs, digit runs, other runs (each with an optional leading
# space), then whitespace that is not followed by a non-space, then any whitespace
SPLIT_PATTERN = r"""'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"""


def byte_table() -> Dict[int, str]:
    """byte -> the one-character symbol GPT-2's vocabulary spells it with: the same table as CLIP's (clip_text.byte_symbols)"""
    return dict(enumerate(byte_symbols()))


def read_merges(path: str) -> Dict[Tuple[str, str], int]:
    """``vocab.bpe``: a version line, then one merge ``a b`` per line in priority order -> pair -> rank (lower merges first)"""
    with open(path, encoding="utf-8") as f:
        lines = f.read().split("\n")
    if lines and lines[0].startswith("#version"):
        lines = lines[1:]
    merges = [tuple(ln.split()) for ln in lines if ln.strip()]
    bad = [m for m in merges if len(m) != 2]
    if bad:
        raise ValueError(f"{path}: a merge line must hold two symbols, got {bad[0]!r}")
    return {m: i for i, m in enumerate(merges)}


class GPT2Vocab:
    def __init__(self, path: str, merges: Optional[str] = None):
        """``path``: encoder.json; ``merges``: vocab.bpe, needed by ``encode`` only"""
        with open(path, encoding="utf-8") as f:
            self.encoder: Dict[str, int] = json.load(f)
        self.decoder = {v: k for k, v in self.encoder.items()}
        self.byte_symbol = byte_table()
        self.byte_decoder = {c: b for b, c in self.byte_symbol.items()}
        self.ranks = None if merges is None else read_merges(merges)
        self._cache: Dict[str, Tuple[str, ...]] = {}
        self._pat = None

    def __len__(self):
        return len(self.encoder)

    def token_id(self, token: str) -> int:
        """the id of ``token`` as ONE vocabulary entry (e.g. the stop token "."); KeyError if it is not a single entry"""
        key = "".join(self.byte_symbol[b] for b in token.encode("utf-8"))
        if key not in self.encoder:
            raise KeyError(f"{token!r} is not a single GPT-2 vocabulary entry")
        return self.encoder[key]

    def decode(self, ids: Iterable[int]) -> str:
        text = "".join(self.decoder[int(i)] for i in ids)
        return bytearray(self.byte_decoder[c] for c in text).decode("utf-8", errors="replace")

    def _merge(self, piece: str) -> Tuple[str, ...]:
        """BPE of one pre-token (in byte symbols): start from single symbols and repeatedly merge every occurrence (left to right)
        of the adjacent pair with the lowest rank until no adjacent pair has one"""
        hit = self._cache.get(piece)
        if hit is not None:
            return hit
        word = list(piece)
        while len(word) > 1:
            best, best_rank = None, None
            for pair in zip(word, word[1:]):
                r = self.ranks.get(pair)
                if r is not None and (best_rank is None or r < best_rank):
                    best, best_rank = pair, r
            if best is None:
                break
            merged, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == best[0] and word[i + 1] == best[1]:
                    merged.append(best[0] + best[1])
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = merged
        out = tuple(word)
        self._cache[piece] = out
        return out

    def encode(self, text: str) -> List[int]:
        """``GPT2Tokenizer.encode(text)``: no markers added, the text taken as it is (case and spaces kept).  KeyError if a merged
        symbol is missing from the vocabulary (the two files do not belong together)."""
        if self.ranks is None:
            raise ValueError("GPT2Vocab.encode needs the merges file (vocab.bpe): GPT2Vocab(encoder_json, merges=...)")
        if self._pat is None:
            import regex     # \p{L} / \p{N} classes (the stdlib ``re`` has none)
            self._pat = regex.compile(SPLIT_PATTERN)
        ids = []
        for tok in self._pat.findall(text):
            piece = "".join(self.byte_symbol[b] for b in tok.encode("utf-8"))
            ids.extend(self.encoder[s] for s in self._merge(piece))
        return ids
