"""Which category next?  Load a saved model (run bert4rec_ml_1m_example.py or bert4rec_lifecycle_example.py first) and ask the app for
each user's probability of picking from every category next (Recommender.category_affinity), a page of shelves ordered by it
(recommend_shelves), and the users of a category campaign (category_audience).  The probabilities are sums of the catalogue softmax
per category, formed on the GPU without a [users, items] matrix.  A synthetic log stands in when the dataset files are absent; the
categories here are made up (the item's token id modulo 12)."""
import argparse
import pathlib

from _common import dataloaders, datasets, models

from bert4rec_amd.apps import Recommender
from bert4rec_amd.models import model_utils

GENRES = ["Action", "Animation", "Comedy", "Crime", "Documentary", "Drama", "Horror", "Musical", "Romance", "Sci-Fi", "Thriller", "Western"]

if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("model", nargs="?", default="bert4rec_ml-1m_lifecycle")
    parser.add_argument("--shelves", type=int, default=3, help="shelves per page")
    parser.add_argument("--k", type=int, default=4, help="items per shelf, users per category")
    parser.add_argument("--users", type=int, default=600, help="users of the campaign")
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
    catalogue = tokenizer.detokenize(list(range(3, tokenizer.get_vocab_size())))
    genre_of = {item: GENRES[(3 + j) % len(GENRES)] for j, item in enumerate(catalogue)}   # made-up categories
    # made-up users: every user has seen a window of the catalogue
    histories = [catalogue[(17 * u) % (len(catalogue) - 40):][:10 + u % 30] for u in range(args.users)]
    names = ["user-%04d" % u for u in range(args.users)]

    for name, row in zip(names[:3], app.category_affinity(histories[:3], genre_of, top=5)):
        print("%s: %s" % (name, ", ".join("%s %.1f %%" % (label, 100 * p) for label, p in row)))
    for name, page in zip(names[:2], app.recommend_shelves(histories[:2], genre_of, shelves=args.shelves, k=args.k)):
        print("the page of %s:" % name)
        for label, p, items in page:
            print("    Top in %s (%.1f %%): %s" % (label, 100 * p, ", ".join(str(i) for i in items)))
    for row in app.category_audience(genre_of, histories, k=args.k, min_probability=0.10, user_ids=names)[:3]:
        print("category %r: %d of %d users pick from it with probability >= 10 %%, expected takers %.1f" %
              (row["label"], row["reach"], args.users, row["expected_demand"]))
        for user, probability in row["users"]:
            print("    %s (probability %.3g)" % (user, probability))
