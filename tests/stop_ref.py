"""Stand-in tokenizers for the stop tests (no tokenizer files are needed): tokens decode to themselves, so HF's `StopStringCriteria`
constructor builds its tables from them as from a real tokenizer, and `KeywordsStoppingCriteria` tokenizes its keywords with them.  The
oracle of every stop test is those two classes run on the CPU over the same id streams (`first_hit`)."""
import torch


class _Encoding(dict):
    """what a tokenizer call returns: ["input_ids"] and .input_ids"""
    __getattr__ = dict.__getitem__


class SelfTokenizer:
    """tokens decode to themselves; text is tokenized by greedy longest match (characters outside the vocabulary are dropped)"""
    bos_token_id = None

    def __init__(self, tokens):
        self.tokens = list(tokens)
        assert len(set(self.tokens)) == len(self.tokens)
        self.vocab = {t: i for i, t in enumerate(self.tokens)}
        self.longest = max(len(t) for t in self.tokens)

    def get_vocab(self):
        return dict(self.vocab)

    def __call__(self, text, add_special_tokens=False, **kw):
        ids, i = [], 0
        while i < len(text):
            for n in range(min(self.longest, len(text) - i), 0, -1):
                t = self.vocab.get(text[i:i + n])
                if t is not None:
                    ids.append(t)
                    i += n
                    break
            else:
                i += 1
        return _Encoding(input_ids=ids)

    def _convert_id_to_token(self, i):
        return self.tokens[i]

    def convert_tokens_to_string(self, tokens):
        return "".join(tokens)

    def ids(self, *tokens):
        return [self.vocab[t] for t in tokens]

    def text(self, ids):
        return "".join(self.tokens[int(i)] for i in ids)


SINGLES = list("abcdef<|>/us r\n")
MULTI = ["ab", "bc", "abc", "cd", "def", "abcdef", "<|", "|>", "user", "us", "er", "</", "s>", "</s", "|user|", ">\n", "<|user|>", "r|>x",
         "xx", "aa", "aba", "bab", "x", "y", "z", "yz", "zy", "xyz"]
VOCAB = ["<unk>", "<s>", "</s>"] + SINGLES + MULTI
STOPS = ["</s>", "<|user|>", "abc", "\n", "ababab"]
QUIET = ["x", "y", "z", "yz", "zy", "xyz", "xx", "d", "e", "f", "def", "cd", " "]


def small_tokenizer():
    return SelfTokenizer(VOCAB)


def fixed_width_tokenizer(vocab_size: int):
    """token i decodes to the unique 7-character string "<%05d>" (id 0: "abcdef", the probe text HF's constructor tokenizes)"""
    return SelfTokenizer(["abcdef"] + ["<%05d>" % i for i in range(1, vocab_size)])


def first_hit(crit, ids) -> int:
    """the first index t at which `crit` returns True on ids[: t + 1], or -1"""
    for t in range(len(ids)):
        r = crit(torch.tensor([list(ids[:t + 1])], dtype=torch.long), None)
        if bool(r.all() if torch.is_tensor(r) else r):
            return t
    return -1


def first_hits_batch(crit, ids: torch.Tensor):
    """ids [rows, T] -> per row the first index at which HF's (batched) criterion returns True on the prefix, or -1"""
    rows, T = ids.shape
    at = torch.full((rows,), -1, dtype=torch.long)
    for t in range(T):
        r = crit(ids[:, :t + 1], None)
        at = torch.where((at < 0) & r.cpu(), torch.full_like(at, t), at)
    return at


def keyword_criterion(seqs, start_length: int):
    """this package's KeywordsStoppingCriteria over given id sequences"""
    from vis_zephyr.model.mm_utils import KeywordsStoppingCriteria
    k = KeywordsStoppingCriteria.__new__(KeywordsStoppingCriteria)
    k.keywords, k.tokenizer = [], None
    k.keyword_ids = [torch.tensor(list(s)) for s in seqs]
    k.max_length = max(len(s) for s in seqs)
    k.start_length = int(start_length)
    return k
