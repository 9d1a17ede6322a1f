"""GPT-2 byte-level token decoding (ids -> text), as ``GPT2Tokenizer.decode`` does it: ids map to vocabulary strings, the
byte-to-unicode table is undone, and the bytes are decoded as UTF-8 with ``errors="replace"``.  Only decoding is restated: captioning
never encodes text (no BPE merges are applied; text prompts are out of scope).  The vocabulary is GPT-2's ``encoder.json`` /
``vocab.json`` (token string -> id); it does not ship with the repository."""
import json
from typing import Dict, Iterable

from .clip_text import byte_symbols


def byte_table() -> Dict[int, str]:
    """byte -> the one-character symbol GPT-2's vocabulary spells it with: the same table as CLIP's (clip_text.byte_symbols)"""
    return dict(enumerate(byte_symbols()))


class GPT2Vocab:
    def __init__(self, path: str):
        with open(path, encoding="utf-8") as f:
            self.encoder: Dict[str, int] = json.load(f)
        self.decoder = {v: k for k, v in self.encoder.items()}
        self.byte_symbol = byte_table()
        self.byte_decoder = {c: b for b, c in self.byte_symbol.items()}

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
