"""Say why an item is recommended ("because you watched X"): load a saved model (run bert4rec_ml_1m_example.py or
bert4rec_lifecycle_example.py first), recommend for a history, and ask the app which history items each recommendation leans on.
One history item at a time is removed on the GPU and the model runs again (Recommender.explain_batch); the reasons are the items
whose removal costs the recommendation the most log probability.  A synthetic log stands in when the dataset files are absent."""
import argparse
import pathlib

from _common import dataloaders, datasets, models

from bert4rec_amd.apps import Recommender
from bert4rec_amd.models import model_utils

if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("model", nargs="?", default="bert4rec_ml-1m_lifecycle")
    parser.add_argument("--k", type=int, default=3, help="recommendations to explain")
    parser.add_argument("--top", type=int, default=2, help="reasons per recommendation")
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
    history = tokenizer.detokenize([7, 19, 4, 33, 12, 25, 41])
    print("history:", history)
    for item, probability, reasons in app.explain(history, k=args.k, top=args.top):
        print("recommended %r (probability %.3g) because of:" % (item, probability))
        for seen, delta in reasons:
            print("    %r: without it the log probability %s by %.3f" % (seen, "falls" if delta >= 0 else "rises", abs(delta)))
    # how far back does the model look?  the two most recent items only
    print("most recent two items only:", app.explain(history, k=1, top=2, window=2)[0])
    # by category: all history items of one (made-up) category are removed together
    shelf = {item: "shelf %d" % (tokenizer.tokenize(item) % 3) for item in history}
    for item, probability, reasons in app.explain(history, k=1, top=3, by_group=shelf):
        for label, delta, n_items in reasons:
            print("%r leans on %s (%d items): %+.3f" % (item, label, n_items, delta))
