"""Several users deciding together: load a saved model (run bert4rec_ml_1m_example.py or bert4rec_lifecycle_example.py first) and ask
the app for one list per party -- a household choosing a film, friends choosing a game (Recommender.recommend_together).  The same
parties under the three strategies: additive (the product of the members' probabilities), least misery (the least happy member
decides) and most pleasure (the happiest member decides), then additive with a veto: nothing a member takes with probability below
0.01 %.  One batched call and one read-back per strategy.  A synthetic log stands in when the dataset files are absent."""
import argparse
import pathlib

from _common import dataloaders, datasets, models

from bert4rec_amd.apps import Recommender
from bert4rec_amd.models import model_utils

if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("model", nargs="?", default="bert4rec_ml-1m_lifecycle")
    parser.add_argument("--k", type=int, default=5, help="items per party")
    args = parser.parse_args()
    path = model_utils.determine_model_path(pathlib.Path(args.model))
    loaded = models.BERT4RecModelWrapper.load(path)
    kwargs = {"tokenizer": loaded["tokenizer"]} if "tokenizer" in loaded else {}
    if not datasets.ML1M.is_available():
        kwargs["data_source"] = datasets.synthetic_dataset(n_users=1500, n_items=3706, min_len=20, max_len=200, seed=0, order=0.6)
    dataloader = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(**kwargs)
    dataloader.generate_vocab()
    app = Recommender(loaded["model_wrapper"].model, dataloader)
    tokenizer = dataloader.get_tokenizer()
    # made-up users: every user has seen a window of the catalogue
    catalogue = tokenizer.detokenize(list(range(3, tokenizer.get_vocab_size())))
    history = lambda u: catalogue[(171 * u) % (len(catalogue) - 40):][:10 + u % 30]  # noqa: E731
    parties = [[history(1), history(2)], [history(3), history(4), history(5), history(6)], [history(7)]]
    for kw in (dict(strategy="additive"), dict(strategy="least_misery"), dict(strategy="most_pleasure"),
               dict(strategy="additive", min_member_probability=1e-4)):
        print(", ".join("%s = %r" % item for item in kw.items()))
        for p, row in enumerate(app.recommend_together(parties, k=args.k, return_members=True, **kw)):
            print("  party %d (%d members)" % (p, len(parties[p])))
            for item, score, probabilities in row:
                print("    %r  score %.3f  members: %s" % (item, score, ", ".join("%.3g" % q for q in probabilities)))
