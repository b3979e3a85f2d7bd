"""Where does this item stand for this user?  Load a saved model (run bert4rec_ml_1m_example.py or bert4rec_lifecycle_example.py first)
and ask the app for the exact position of given items in each user's full-catalogue ranking (Recommender.item_ranks: "X is at 312 of
3 700 for this user"), then evaluate the model on the next-n protocol: the last n items of every sequence are held out and Recall@k,
NDCG@k, MAP@k, MRR and AUC follow from their exact ranks (evaluation.get(full_ranking=True, multi_target=True)).  The ranks come from
one sweep over the catalogue on the GPU, whatever the number of items asked about.  A synthetic log stands in when the dataset files
are absent."""
import argparse
import pathlib

from _common import dataloaders, datasets, evaluation, models

from bert4rec_amd.apps import Recommender
from bert4rec_amd.models import model_utils

if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("model", nargs="?", default="bert4rec_ml-1m_lifecycle")
    parser.add_argument("--n", type=int, default=3, help="held-out items per user")
    parser.add_argument("--users", type=int, default=600, help="users of the evaluation")
    args = parser.parse_args()
    path = model_utils.determine_model_path(pathlib.Path(args.model))
    loaded = models.BERT4RecModelWrapper.load(path)
    kwargs = {"tokenizer": loaded["tokenizer"]} if "tokenizer" in loaded else {}
    if not datasets.ML1M.is_available():
        kwargs["data_source"] = datasets.synthetic_dataset(n_users=1500, n_items=3706, min_len=20, max_len=200, seed=0, order=0.6)
    dataloader = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(**kwargs)
    dataloader.generate_vocab()
    model = loaded["model_wrapper"].model
    app = Recommender(model, dataloader)
    tokenizer = dataloader.get_tokenizer()
    catalogue = tokenizer.detokenize(list(range(3, tokenizer.get_vocab_size())))
    # made-up users: every user has seen a window of the catalogue
    histories = [catalogue[(17 * u) % (len(catalogue) - 40):][:10 + u % 30] for u in range(args.users)]

    # a promoted item, a cart item the user has already seen, and an item the vocabulary does not know
    asked = [catalogue[100], histories[0][0], "no such item"]
    for u, row in enumerate(app.item_ranks(histories[:3], items=asked)):
        for entry in row:
            where = "not served" if entry["rank"] is None else "at %d of %d (top %.1f %%)" % (entry["rank"], entry["of"], 100.0 * entry["rank"] / entry["of"])
            print("user-%04d: %r stands %s" % (u, entry["item"], where))

    batches, skipped = evaluation.next_n_batches(dataloader, histories, args.n)
    evaluator = evaluation.get(full_ranking=True, multi_target=True)
    evaluator.evaluate(model, batches)
    print("next-%d evaluation of %d users (%d too short):" % (args.n, args.users - skipped, skipped))
    for name, value in evaluator.get_metrics_results().items():
        print("    %-12s %s" % (name, value if isinstance(value, int) else "%.4f" % value))
