"""Single-sequence recommendation (the reference's demo app, bert4rec/apps/recommender.py:14-63): append a masked slot to the
history (prepare_inference), score the whole vocabulary for that slot and return the best item(s) the user has not seen.

On the GPU this is the evaluation path: encoder forward, tfm MaskedLM's transform on the ONE masked slot, one
b4r_rank_candidates call over the whole vocabulary (cand = NULL: no [1, V] candidate list, no [B, P, V] logits).  Deliberate
differences from the reference, both documented in INTEGRATION.md: it reads ``mlm_logits[:, -1]``, i.e. the LAST of the P slots
-- a padded slot that gathers position 0 -- where the masked token sits in slot 0 (used here); and it can return [PAD] / [MASK] /
[UNK], which are excluded here together with the seen items.

recommend_batch serves many users at once: one forward over the stacked batch and one b4r_rank_full call (the best k allowed items of
every user in one sweep over the vocabulary, no [users, V] scores, the seen items excluded on the device)."""
import numpy as np
import torch


class Recommender:
    def __init__(self, model, dataloader):
        self.model = model
        self.dataloader = dataloader

    def __call__(self, sequence: list, k: int = 1):
        tokenizer = self.dataloader.get_tokenizer()
        batch = self.dataloader.prepare_inference(list(sequence))
        batch = {key: torch.from_numpy(np.asarray(v)) for key, v in batch.items()}
        blocked = set(tokenizer.tokenize(list(sequence))) | {0, 1, 2}
        ranking, _, _, _ = self.model.rank_items_tensor(batch, None)      # [1, V]: the whole vocabulary, best first
        # the best k ids outside `blocked` are among the first k + |blocked| entries
        head = ranking[0, :k + len(blocked)].cpu().tolist()
        top = [i for i in head if i not in blocked][:k]
        items = tokenizer.detokenize(top)
        return items[0] if k == 1 else items

    def recommend_batch(self, sequences, k: int = 1) -> list:
        """Recommender(...)(seq, k) for every sequence of `sequences`, from one batched forward and one full-catalogue top-k."""
        tokenizer = self.dataloader.get_tokenizer()
        sequences = [list(seq) for seq in sequences]
        if not sequences:
            return []
        batches = [self.dataloader.prepare_inference(list(seq)) for seq in sequences]
        batch = {key: torch.from_numpy(np.concatenate([np.asarray(b[key]) for b in batches], axis=0)) for key in batches[0]}
        seen = [tokenizer.tokenize(seq) for seq in sequences]
        width = max(1, max(len(t) for t in seen))
        exclude = torch.full((len(seen), width), -1, dtype=torch.int64)
        for i, t in enumerate(seen):
            if t:
                exclude[i, :len(t)] = torch.as_tensor(t, dtype=torch.int64)
        ids, _, slots = self.model.recommend_tensor(batch, k=k, exclude_seen=False, exclude=exclude)
        P = int(batch["masked_lm_positions"].shape[1])
        first = {}
        for i, s in enumerate(slots.cpu().tolist()):   # __call__ ranks the first weighted slot of its one-row batch
            first.setdefault(s // P, i)
        ids_h = ids.cpu().tolist()
        out = []
        for b in range(len(sequences)):
            top = [i for i in ids_h[first[b]] if i >= 0] if b in first else []
            items = tokenizer.detokenize(top)
            out.append(items[0] if k == 1 else items)
        return out
