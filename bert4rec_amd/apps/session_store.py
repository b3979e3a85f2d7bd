"""Session store: the users' histories stay on the device, next to the model.  An event appends one item to one user's history
(b4r_history_append), a request names users (b4r_history_batch builds their batch rows and exclusion lists on the device), so that a
serving call no longer tokenises, prepares and uploads every user's whole history:

    sessions = recommender.open_sessions(max_users=100_000)
    sessions.append(["ann", "bob", "ann"], ["Heat (1995)", "Alien (1979)", "Ronin (1998)"])     # three events, in order
    sessions.recommend(["ann", "bob", "new user"], k=10)                                        # recommend_batch's lists

A user key is any hashable; the host keeps key -> row in a dict.  A user the store has never seen is a cold user: the model sees the
lone [MASK] placeholder, as recommend_batch([[]]) does.

Exclusions.  A user's history is a ring of `history_capacity` items on the device (default max(max_seq_len - 1, 256)): the model's
window reads the most recent max_seq_len - 1 of them, and the user's exclusions are the last `history_capacity` items.  That is the
full history as long as it is no longer than the capacity; recommend_batch always excludes the full history, so for a longer
history an item older than the last `history_capacity` events may be recommended again."""
import torch

from .. import engine as engine_mod
from ..engine import MASK_ID, SPECIAL_IDS

UNK_ID = 2   # what prepare_inference leaves in masked_lm_ids under the placeholder


def default_history_capacity(max_seq_len: int) -> int:
    return max(int(max_seq_len) - 1, 256)


def check_session_args(max_users, history_capacity, max_seq_len: int):
    """Argument checks of a session store that need no GPU.  history_capacity None: max(max_seq_len - 1, 256); a capacity below
    max_seq_len - 1 could not fill the model's window and raises ValueError.  Returns (max_users, history_capacity)."""
    if history_capacity is None:
        history_capacity = default_history_capacity(max_seq_len)
    max_users, capacity = engine_mod.check_history_state_args(max_users, history_capacity)
    if capacity < int(max_seq_len) - 1:
        raise ValueError(f"history_capacity = {capacity} is below max_seq_len - 1 = {int(max_seq_len) - 1}: the model's window would "
                         f"never fill")
    return max_users, capacity


class SessionStore:
    """Recommender.open_sessions(max_users, history_capacity=None).  See the module's docstring for the exclusions of a history that is
    longer than history_capacity."""

    def __init__(self, recommender, max_users: int, history_capacity=None):
        self.recommender = recommender
        dl = recommender.dataloader
        self.max_seq_len, self.max_predictions = int(dl._MAX_SEQ_LENGTH), int(dl._MAX_PREDICTIONS_PER_SEQ)
        self.max_users, self.history_capacity = check_session_args(max_users, history_capacity, self.max_seq_len)
        engine_mod._int_in(self.max_seq_len, 2, engine_mod.HISTORY_MAX_LEN, "max_seq_len")
        self.engine = recommender.model.engine
        self.state = self.engine.history_state(self.max_users, self.history_capacity)
        self._rows = {}          # user key -> row
        self._free = []          # rows given back by forget, reused last in first out
        self._next_row = 0       # rows below it have been handed out

    # ---- users ----------------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return len(self._rows)

    def _rows_of(self, user_keys) -> torch.Tensor:
        """The row of every key, int32 [n] on the device; -1 for a user the store does not hold"""
        rows = [self._rows.get(key, -1) for key in user_keys]
        return torch.tensor(rows, dtype=torch.int32).to(self.engine.device)

    def _assign_rows(self, user_keys) -> list:
        """The row of every key; a new key takes the next free row.  A store too full for all of them raises before any is taken."""
        new = []
        seen = set()
        for key in user_keys:
            if key not in self._rows and key not in seen:
                seen.add(key)
                new.append(key)
        room = len(self._free) + self.max_users - self._next_row
        if len(new) > room:
            raise ValueError(f"the session store is full: {len(new)} new users, room for {room} of {self.max_users}")
        for key in new:
            if self._free:
                self._rows[key] = self._free.pop()
            else:
                self._rows[key] = self._next_row
                self._next_row += 1
        return [self._rows[key] for key in user_keys]

    # ---- events ---------------------------------------------------------------------------------------------------------------------
    def append(self, user_keys, items, return_accepted: bool = True):
        """One event per (user key, item) pair, in order.  Only the new items are tokenised; an item the vocabulary does not know is
        dropped (and never added to the vocabulary).  Returns the number of accepted events -- one read-back; return_accepted=False
        reads nothing back and returns None."""
        user_keys, items = list(user_keys), list(items)
        if len(user_keys) != len(items):
            raise ValueError(f"{len(user_keys)} user keys for {len(items)} items")
        if len(items) > engine_mod.HISTORY_MAX_EVENTS:
            raise ValueError(f"at most {engine_mod.HISTORY_MAX_EVENTS} events per call, got {len(items)}")
        if not items:
            return 0 if return_accepted else None
        tokens = self.recommender._token_ids(items)      # -1: unknown, which b4r_history_append drops
        rows = torch.tensor(self._assign_rows(user_keys), dtype=torch.int32)
        dev = self.engine.device
        rows_d, tokens_d = rows.to(dev), tokens.to(dev)
        accepted = torch.empty((len(items),), dtype=torch.int32, device=dev) if return_accepted else None
        self.append_rows(rows_d, tokens_d, accepted)
        return int(accepted.sum()) if return_accepted else None

    def append_rows(self, rows: torch.Tensor, token_ids: torch.Tensor, accepted=None) -> None:
        """The events as device tensors: rows int32 [N] (the users' rows in the store), token_ids int64 [N], in order; accepted
        (optional) int32 [N] receives 1 / 0 per event; at most 65 536 events per call.  No host work and no synchronisation."""
        self.engine.history_append(self.state, rows, token_ids, accepted, first_item=SPECIAL_IDS)

    def forget(self, user_keys) -> None:
        """Zeroes the users' counts and frees their rows; a key the store does not hold is ignored."""
        rows = []
        for key in user_keys:
            row = self._rows.pop(key, None)
            if row is not None:
                rows.append(row)
        if rows:
            self.state["count"][torch.tensor(rows, dtype=torch.int64).to(self.engine.device)] = 0
            self._free.extend(rows)

    def history(self, user_key) -> list:
        """The items held for the user, oldest first (at most history_capacity of them): one read-back."""
        row = self._rows.get(user_key)
        if row is None:
            return []
        C = self.history_capacity
        both = torch.cat([self.state["count"][row:row + 1], self.state["hist"][row]]).cpu().tolist()
        n, ring = both[0], both[1:]
        held = min(n, C)
        return self.recommender.dataloader.get_tokenizer().detokenize([ring[(n - held + i) % C] for i in range(held)])

    # ---- requests -------------------------------------------------------------------------------------------------------------------
    def requests(self, user_keys):
        """(batch, exclude) in the form Recommender._requests returns -- input_word_ids, input_mask, masked_lm_positions,
        masked_lm_weights, masked_lm_ids and exclude [n, history_capacity] int64, -1 padded -- but on the device, built there from the
        store (prepare_inference's `labels`, the unmasked row, is not formed: no inference call reads it).  An unknown user key is a
        cold user: the lone placeholder."""
        user_keys = list(user_keys)
        got = self.engine.history_batch(self.state, self._rows_of(user_keys), self.max_seq_len, self.max_predictions, self.history_capacity,
                                        mask_id=MASK_ID)
        ids = torch.zeros_like(got["positions"])
        ids[:, 0] = UNK_ID
        batch = {"input_word_ids": got["tokens"], "input_mask": got["mask"], "masked_lm_positions": got["positions"],
                 "masked_lm_weights": got["weights"], "masked_lm_ids": ids}
        return batch, got["exclude"]

    def recommend(self, user_keys, k: int = 1, allowed_items=None, allowed_items_per_user=None, diversity=None, candidate_pool=None,
                  max_per_group=None, return_probabilities: bool = False, min_probability=None, temperature: float = 1.0,
                  sample_seed=None, user_streams=None, calibrate_by=None, calibrate_to: str = "history", calibration=None) -> list:
        """Recommender.recommend_batch for the users' stored histories: every keyword means what it means there and the values
        returned are the same, as long as no history is longer than history_capacity (see the module's docstring)."""
        user_keys = list(user_keys)
        rec = self.recommender
        serve = rec._recommend_options(len(user_keys), k, allowed_items, allowed_items_per_user, diversity, candidate_pool, max_per_group,
                                       return_probabilities, min_probability, temperature, sample_seed, user_streams, calibrate_by,
                                       calibrate_to, calibration)
        if not user_keys:
            return []
        batch, exclude = self.requests(user_keys)
        return rec._recommend_requests(batch, exclude, len(user_keys), serve)

    def allocate(self, user_keys, stock, k: int = 10, candidate_pool=None, allowed_items=None, user_ids=None,
                 return_probabilities: bool = True):
        """Recommender.allocate for the users' stored histories: limited items (`stock`: item -> units) are shared out among the
        users of the call; every keyword means what it means there and the values returned are the same, as long as no history is
        longer than history_capacity (see the module's docstring)."""
        user_keys = list(user_keys)
        rec = self.recommender
        serve = rec._allocate_options(len(user_keys), stock, k, candidate_pool, allowed_items, user_ids, return_probabilities)
        if not user_keys:
            return [], dict(serve["left"])
        batch, exclude = self.requests(user_keys)
        return rec._allocate_requests(batch, exclude, len(user_keys), serve)

    # ---- persistence ----------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """CPU tensors plus the key list, so that a store survives a restart: hist / count of the rows handed out so far, keys[i] /
        rows[i] the users."""
        n = self._next_row
        keys = list(self._rows)
        return {"hist": self.state["hist"][:n].cpu(), "count": self.state["count"][:n].cpu(), "keys": keys,
                "rows": torch.tensor([self._rows[key] for key in keys], dtype=torch.int64), "history_capacity": self.history_capacity}

    def load_state_dict(self, sd: dict) -> None:
        """Replaces what the store holds by a state_dict() of a store with the same history_capacity and no more rows than max_users."""
        hist, count, keys = torch.as_tensor(sd["hist"]), torch.as_tensor(sd["count"]), list(sd["keys"])
        rows = torch.as_tensor(sd["rows"]).to(torch.int64).reshape(-1).tolist()
        n = int(count.numel())
        if int(sd["history_capacity"]) != self.history_capacity or hist.dtype != torch.int64 or count.dtype != torch.int64 or \
                tuple(hist.shape) != (n, self.history_capacity) or count.ndim != 1:
            raise ValueError(f"the saved store does not fit: hist {tuple(hist.shape)} {hist.dtype}, count {tuple(count.shape)} {count.dtype}, "
                             f"capacity {sd['history_capacity']} against [{n}, {self.history_capacity}] int64")
        if n > self.max_users:
            raise ValueError(f"the saved store holds {n} rows, this one at most {self.max_users}")
        if len(keys) != len(rows) or len(set(rows)) != len(rows) or len(set(keys)) != len(keys) or any(r < 0 or r >= n for r in rows):
            raise ValueError("the saved store's keys and rows disagree")
        dev = self.engine.device
        self.state["count"].zero_()
        self.state["count"][:n] = count.to(dev)
        self.state["hist"][:n] = hist.to(dev)
        self._rows = dict(zip(keys, rows))
        self._next_row = n
        used = set(rows)
        self._free = [r for r in range(n) if r not in used]
        if self._free:
            self.state["count"][torch.tensor(self._free, dtype=torch.int64).to(dev)] = 0
