"""Given an item, which users?  Load a saved model (run bert4rec_ml_1m_example.py or bert4rec_lifecycle_example.py first) and ask the
app for the users most likely to take each of a few items next, how many users reach a probability of 1 %, and the demand to expect
(Recommender.audience).  The users go through the model in batches; the k best users of every item stay on the GPU while the batches
go by and are read back once.  A synthetic log stands in when the dataset files are absent."""
import argparse
import pathlib

from _common import dataloaders, datasets, models

from bert4rec_amd.apps import Recommender
from bert4rec_amd.models import model_utils

if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("model", nargs="?", default="bert4rec_ml-1m_lifecycle")
    parser.add_argument("--k", type=int, default=5, help="users per item")
    parser.add_argument("--users", type=int, default=600, help="users to choose among")
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
    histories = [catalogue[(17 * u) % (len(catalogue) - 40):][:10 + u % 30] for u in range(args.users)]
    names = ["user-%04d" % u for u in range(args.users)]
    items = tokenizer.detokenize([7, 19, 400])
    for item, row in zip(items, app.audience(items, histories, k=args.k, min_probability=0.01, user_ids=names, batch_size=256)):
        print("item %r: %d of %d users would take it with probability >= 1 %%, expected demand %.2f" %
              (item, row["reach"], args.users, row["expected_demand"]))
        for user, probability in row["users"]:
            print("    %s (probability %.3g)" % (user, probability))
