"""CLIP's byte-level BPE tokenizer and RegionCLIP's prompt engineering, restated for the concept-embedding tool
(detectron2/data/datasets/clip_prompt_utils.py:22-140 ``SimpleTokenizer``, :170-352 templates / ``prompt_engineering`` /
``convert_example_to_features_bpe`` / ``pre_tokenize``).

Neither the BPE vocabulary nor the template list ships with this package: both are inputs (CLIP's
``bpe_simple_vocab_16e6.txt.gz`` and a text file with one template per line).

Text clean-up: the reference runs ``ftfy.fix_text`` first.  ftfy is not a dependency here, so only its other two steps are
kept (``html.unescape`` twice, then whitespace clean-up and lower-casing).  For text that ``ftfy.fix_text`` leaves unchanged
(plain ASCII, well-formed Unicode) the ids are the reference's; for text it would change (mojibake, odd quotes, ...)
parity is not pinned.
"""
import gzip
import html
from typing import Dict, List, Sequence, Tuple, Union

import torch

CONTEXT_LENGTH = 77
SOT, EOT = "<|startoftext|>", "<|endoftext|>"
N_MERGES = 49152 - 256 - 2            # merges CLIP keeps from the vocab file (48 894)


def byte_symbols() -> List[str]:
    """The 256 one-character symbols CLIP's BPE works on, in byte order: printable Latin-1 bytes stand for themselves, the
    other 68 (controls, space, soft hyphen, ...) are moved to code points 256, 257, ... in the order they occur."""
    keep = set(range(0x21, 0x7F)) | set(range(0xA1, 0xAD)) | set(range(0xAE, 0x100))
    out, shifted = [], 0
    for b in range(256):
        if b in keep:
            out.append(chr(b))
        else:
            out.append(chr(256 + shifted))
            shifted += 1
    return out


def token_order() -> List[str]:
    """CLIP's base vocabulary, in id order: the byte symbols sorted as CLIP lists them (the kept printable bytes first, then the
    shifted ones), and the same 256 again with the end-of-word marker."""
    sym = byte_symbols()
    kept = [b for b in range(256) if ord(sym[b]) == b]
    moved = [b for b in range(256) if ord(sym[b]) != b]
    base = [sym[b] for b in kept + moved]
    return base + [s + "</w>" for s in base]


def _pretokenizer():
    import regex     # \p{L} / \p{N} classes (the stdlib ``re`` has none)
    contractions = "|".join("'" + c for c in ("s", "t", "re", "ve", "m", "ll", "d"))
    specials = "|".join(regex.escape(s) for s in (SOT, EOT))
    return regex, regex.compile(rf"{specials}|{contractions}|\p{{L}}+|\p{{N}}|[^\s\p{{L}}\p{{N}}]+", regex.IGNORECASE)


class BPETokenizer:
    """Text -> CLIP token ids.  ``ranks`` maps a symbol pair to its merge priority (lower merges first), ``vocab`` a symbol to its
    id; the two specials must be in ``vocab``."""

    def __init__(self, ranks: Dict[Tuple[str, str], int], vocab: Dict[str, int]):
        self.ranks, self.vocab = dict(ranks), dict(vocab)
        self.sot, self.eot = self.vocab[SOT], self.vocab[EOT]
        self._bytes = byte_symbols()
        self._re, self._pat = _pretokenizer()
        self._ws = self._re.compile(r"\s+")
        self._cache = {SOT: (SOT,), EOT: (EOT,)}

    @classmethod
    def from_vocab_file(cls, path):
        """CLIP's ``bpe_simple_vocab_16e6.txt.gz``: a version line, then one merge ``a b`` per line in priority order.  Ids: the 256
        byte symbols, the same with ``</w>``, the first 48 894 merges in file order, then ``<|startoftext|>``, ``<|endoftext|>``.
        (Blank lines are skipped; the real file has none in the range read.)"""
        with gzip.open(path, "rt", encoding="utf-8") as f:
            lines = f.read().split("\n")[1:]
        merges = [tuple(ln.split()) for ln in lines if ln.strip()][:N_MERGES]
        order = token_order() + ["".join(m) for m in merges] + [SOT, EOT]
        return cls({m: i for i, m in enumerate(merges)}, {s: i for i, s in enumerate(order)})

    @classmethod
    def from_tables(cls, ranks: Dict[Tuple[str, str], int], vocab: Dict[str, int]):
        """explicit tables (e.g. a pruned subset of CLIP's that still covers the text to be encoded)"""
        return cls(ranks, vocab)

    def _merge(self, piece: str) -> Tuple[str, ...]:
        """BPE of one pre-token (already in byte symbols): start from single symbols, the last carrying ``</w>``, and repeatedly
        merge every occurrence (left to right) of the adjacent pair with the lowest rank until no adjacent pair has one."""
        if piece in self._cache:
            return self._cache[piece]
        word = list(piece[:-1]) + [piece[-1] + "</w>"]
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
        """ids of ``text`` without the start / end markers"""
        text = self._ws.sub(" ", html.unescape(html.unescape(text)).strip()).strip().lower()
        ids = []
        for tok in self._pat.findall(text):
            piece = "".join(self._bytes[b] for b in tok.encode("utf-8"))
            ids.extend(self.vocab[s] for s in self._merge(piece))
        return ids

    def encode_padded(self, text: str, context_length: int = CONTEXT_LENGTH) -> List[int]:
        """``convert_example_to_features_bpe``: [SOT] + ids + [EOT], cut to ``context_length`` (the cut can drop the EOT), padded
        with id 0"""
        ids = ([self.sot] + self.encode(text) + [self.eot])[:context_length]
        return ids + [0] * (context_length - len(ids))


def read_templates(path) -> List[str]:
    """one prompt template per non-empty line, each holding ``{}`` where the class name goes"""
    with open(path, encoding="utf-8") as f:
        out = [ln.rstrip("\n") for ln in f if ln.strip()]
    for t in out:
        if "{}" not in t:
            raise ValueError(f"template without '{{}}': {t!r}")
    return out


def prompt_engineering(name: str, template: str) -> str:
    """the reference's rule: drop ',' from the name, turn '+' into a space, put it where '{}' is"""
    return template.replace("{}", name.replace(",", "").replace("+", " "))


def concept_prompts(name: Union[str, Sequence[str]], templates: Sequence[str]) -> List[str]:
    """every template for every synonym (``pre_tokenize``: a name may be one string or a list of synonyms)"""
    names = [name] if isinstance(name, str) else list(name)
    return [prompt_engineering(v, t) for v in names for t in templates]


def tokenize_prompts(prompts: Sequence[str], bpe: BPETokenizer, context_length: int = CONTEXT_LENGTH) -> torch.Tensor:
    """[len(prompts), context_length] int64"""
    return torch.tensor([bpe.encode_padded(p, context_length) for p in prompts], dtype=torch.int64).view(-1, context_length)


def tokenize_concepts(names, templates: Sequence[str], bpe: BPETokenizer, context_length: int = CONTEXT_LENGTH) -> torch.Tensor:
    """``pre_tokenize``: [C, P, context_length] int64, P = synonyms x templates (the same for every class, as the reference's
    stack requires)"""
    per = [tokenize_prompts(concept_prompts(n, templates), bpe, context_length) for n in names]
    if len({p.shape[0] for p in per}) > 1:
        raise ValueError("classes have different numbers of prompts (synonym counts differ); use encode_concepts, which takes them")
    return torch.stack(per, 0)
